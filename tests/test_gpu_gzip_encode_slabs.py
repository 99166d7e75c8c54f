"""zh_gzip_encode_batch over a batch that crosses a slab boundary: the batch level of
test_gpu_gzip_encode.py, whose helpers this uses, at the one size where the slab cutter acts."""
import zlib

import pytest

import gzip_enc_inputs as gi
from test_gpu_gzip_encode import Uploaded

pytestmark = pytest.mark.gpu


def test_batch_of_several_slabs(dev):
    """More than 128 MiB of raw input in one batch: the call works slab by slab (block and job
    indexes, device offsets and the running place in the destination restart in every slab; the
    CRCs are the batch's).  Two buffers of 70 MiB of a short byte ramp between two small ones make
    the slabs [c, A] and [B, d]; every member equals the member of a one-member batch over the
    same device bytes (which test_gpu_gzip_encode.py holds to the host writer)."""
    big = 70 << 20
    a = (bytes(range(251)) * (big // 251 + 1))[:big]
    b = (bytes(range(3, 244)) * (big // 241 + 1))[:big]
    buffers = [gi.high_bytes(), a, b, gi.random_bytes(3001)]
    assert len(buffers[0]) + len(a) <= 128 << 20 < len(buffers[0]) + len(a) + len(b)
    up = Uploaded(dev, buffers)
    try:
        out, rows = dev.gzip_encode_batch_raw(up.sources, 0)
        members = [bytes(out[o:o + n]) for o, n in rows]
        for k, src in enumerate(up.sources):
            one, ((o, n),) = dev.gzip_encode_batch_raw([src], 0)
            assert members[k] == bytes(one[o:o + n]), k
    finally:
        up.free()
    end = 0
    for (o, n), buf in zip(rows, buffers):  # in order, 16-byte aligned, never overlapping: across
        assert o >= end and o % 16 == 0 and 20 <= n <= gi.bound(len(buf), 0)    # the slabs too
        end = o + n
    assert end <= len(out)
    for k, (f, buf) in enumerate(zip(members, buffers)):
        assert zlib.decompress(f, 31) == buf, k
