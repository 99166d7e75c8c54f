"""bench.py --dump-outputs: the sampler (bench.dump_outputs) on a host stand-in for the device
buffer: the same runs every time, inside the buffer, first and last run included, exact values,
and a file well under the 64 MB a dump may take."""
import os

import numpy as np


class _HostBuffer:
    """d2h of a numpy array addressed from 0, refusing reads outside it."""

    def __init__(self, a):
        self.a = a.view(np.uint8)

    def d2h(self, src, nbytes):
        assert 0 <= src and src + nbytes <= self.a.size and src % 4 == 0
        return self.a[src:src + nbytes].tobytes()


def test_dump_outputs_sample_is_fixed_exact_and_bounded(tmp_path):
    import bench
    nel = 1024 * 4096 + 5 * 4096  # just more than the sample, a whole number of runs
    a = (np.arange(nel, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    a[-1] = 0xFFFFFFFF  # float32 could not hold it
    info = bench.dump_outputs(_HostBuffer(a), 0, nel, str(tmp_path / "d1"))
    bench.dump_outputs(_HostBuffer(a), 0, nel, str(tmp_path / "d2"))
    assert os.listdir(tmp_path / "d1") == ["decoded_sample.npy"]
    x = np.load(tmp_path / "d1" / "decoded_sample.npy")
    assert x.dtype == np.float64 and list(x.shape) == info["shape"] == [1024, 4096]
    assert x.nbytes <= 64 * 1000 * 1000
    assert np.array_equal(x, np.load(tmp_path / "d2" / "decoded_sample.npy"))
    assert np.array_equal(x[0], a[:4096]) and np.array_equal(x[-1], a[-4096:])
    assert x[-1, -1] == 0xFFFFFFFF
    runs = {r.tobytes() for r in a.reshape(-1, 4096).astype(np.float64)}
    assert all(r.tobytes() in runs for r in x)  # every row is one aligned run of the array


def test_dump_outputs_small_array_whole(tmp_path):
    import bench
    a = np.arange(1000, dtype=np.uint32)[::-1].copy()
    bench.dump_outputs(_HostBuffer(a), 0, a.size, str(tmp_path))
    assert np.array_equal(np.load(tmp_path / "decoded_sample.npy"), a.reshape(1, -1))
