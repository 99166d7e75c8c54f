"""zh_blosc_encode_batch (flags 0) over a batch that crosses a slab boundary: the batch level of
test_gpu_blosc_encode.py, whose helpers this uses, at the one size where the slab cutter acts."""
import pytest

import blosc_enc_inputs as bi
from test_gpu_blosc_encode import Uploaded, decode

pytestmark = pytest.mark.gpu


def test_batch_of_several_slabs(dev):
    """More than 128 MiB of raw input in one batch: the call works slab by slab (block, stream and
    job indexes, device offsets and the running place in the destination restart in every slab).
    Two buffers of 70 MiB of a short byte ramp between two small ones make the slabs [c, A] and
    [B, d]; every frame equals the frame of a one-frame batch over the same device bytes (which
    test_gpu_blosc_encode.py holds to the host writer), and the frames decode back to the
    buffers."""
    big = 70 << 20
    a = (bytes(range(251)) * (big // 251 + 1))[:big]
    b = (bytes(range(3, 244)) * (big // 241 + 1))[:big]
    buffers = [bi.smooth(5000), a, b, bi.smooth(3001)]
    assert len(buffers[0]) + len(a) <= 128 << 20 < len(buffers[0]) + len(a) + len(b)
    up = Uploaded(dev, buffers)
    try:
        out, rows = dev.blosc_encode_batch_raw(up.sources, 4, 1, 0)
        frames = [bytes(out[o:o + n]) for o, n in rows]
        for k, src in enumerate(up.sources):
            one, ((o, n),) = dev.blosc_encode_batch_raw([src], 4, 1, 0)
            assert frames[k] == bytes(one[o:o + n]), k
    finally:
        up.free()
    end = 0
    for o, n in rows:           # in order, 16-byte aligned, never overlapping: across the slabs too
        assert o >= end and o % 16 == 0 and n >= 16
        end = o + n
    assert end <= len(out)
    assert [f[2] & 0x02 for f in frames] == [0] * 4        # compressed, none MEMCPYED
    assert decode(dev, frames) == buffers
