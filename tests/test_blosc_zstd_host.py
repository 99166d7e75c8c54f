"""The host half of the device decode of blosc frames with zstd streams (ZH_BLOSC_ZSTD_DEVICE:
zh_blosc_batch_plan_ex, zh_debug_blosc_streams_ex, zarr-java_amd/csrc/zh_blosc_streams.h): the
plan and the stream table with and without the flag, and the route's host-side logic (plan, rows,
the zstd frame decoder on one lane, the unshuffle) under AddressSanitizer + UBSan in a stand-alone
program over the valid matrix and the corrupt frames.  No GPU."""
import os
import shutil
import struct
import subprocess

import pytest

import blosc_frames as bf
import blosc_zstd_inputs as zi
from zarrhip import _abi as A
from zarrhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan and the stream table ----------------------------------------------------------------
def test_matrix_is_planned_for_the_device_only_with_the_flag():
    assert A.ZH_BLOSC_ZSTD_DEVICE == zi.FLAG
    for label, data, f in zi.matrix():
        st, out, msg = bf.host_decode(f)
        assert (st, out) == (bf.ZH_OK, data), (label, msg)
        total, rows = _lib.blosc_batch_plan([f], zi.FLAG)
        assert rows == [(0, len(data), 0)] and total == -(-len(data) // 256) * 256, label
        assert _lib.blosc_batch_plan([f]) == (total, [(0, len(data), 1)]), label
        assert _lib.blosc_batch_plan([f], 0) == (total, [(0, len(data), 1)]), label
        # without the flag the table refuses the frame exactly as it always has
        with pytest.raises(_lib.ZhError) as e:
            _lib.blosc_streams(f)
        assert (e.value.status, str(e.value)) == (bf.ZH_EUNSUPPORTED,
                                                  "blosc payload is decoded on the host"), label


def walk(f):
    """The block / stream rows of a zstd frame by a walk written here."""
    ver, flags, ts = f[0], f[2], f[3]
    nbytes, blocksize, _ = struct.unpack("<III", f[4:16])
    nblocks = -(-nbytes // blocksize) if nbytes else 0
    starts = struct.unpack(f"<{nblocks}I", f[16:16 + 4 * nblocks])
    if flags & 0x04 and not flags & 0x01:
        shuffle = 2 if ver <= 2 else 3
    else:
        shuffle = 1 if flags & 0x01 and ts > 1 else 0
    rows = []
    for b in range(nblocks):
        bsize = min(blocksize, nbytes - b * blocksize)
        nsplit = 1 if flags & 0x10 or bsize < blocksize else ts
        rows.append((0, b * blocksize, bsize, ts, shuffle, nsplit))
        pos = starts[b]
        for s in range(nsplit):
            (cs,) = struct.unpack("<i", f[pos:pos + 4])
            pos += 4
            want = bsize // nsplit
            rows.append((1, pos, cs, s * want, want, 0 if cs == want else zi.KZSTD))
            pos += cs
    return rows


def test_stream_table_with_the_flag():
    seen = set()
    for label, data, f in zi.matrix():
        rows = _lib.blosc_streams(f, zi.FLAG)
        assert rows == walk(f), label
        for r in rows:
            seen.add(("block", r[4], r[5], r[2] > zi.LDS_BLOCK) if r[0] == 0 else ("stream", r[5]))
    blocks = {k[1:] for k in seen if k[0] == "block"}
    assert {k[1] for k in seen if k[0] == "stream"} == {0, zi.KZSTD}
    assert {b[0] for b in blocks} == {0, 1, 2, 3}            # every shuffle kind
    assert {b[1] for b in blocks} == {1, 4, 8}               # unsplit, 4 and 8 streams
    assert (1, 1, True) in blocks and (0, 1, True) in blocks  # blocks beyond the LDS window
    # the split block of `quad`: a raw stream, then three zstd frames
    f = next(f for lb, _, f in zi.matrix() if lb.startswith("split, raw and constant"))
    assert [r[5] for r in _lib.blosc_streams(f, zi.FLAG) if r[0] == 1] == [0, 3, 3, 3]
    # LZ4 / BloscLZ frames: the same table with the flag as without
    for label, f in bf.matrix()[::17]:
        assert _lib.blosc_streams(f, zi.FLAG) == _lib.blosc_streams(f), label


def test_matrix_covers_the_entropy_paths():
    """The inputs cannot silently stop reaching Huffman-4-stream literals, FSE-mode tables, a
    stream of several zstd blocks, RLE blocks and repeated tables."""
    pytest.importorskip("pyarrow")
    huf4 = fse = multi = rle = False
    for label, data, f in zi.matrix():
        for s in zi.zstd_streams(f):
            rows = _lib.zstd_blocks(s)
            multi |= len(rows) > 1
            for r in rows:
                rle |= r[0] == 1
                huf4 |= r[0] == 2 and r[3] == 2 and r[4] == 4
                fse |= r[0] == 2 and r[6] > 0 and 2 in r[7:10]
    assert huf4 and fse and multi and rle


def test_host_routed_and_mixed_frames():
    for label, data, f in zi.host_routed():
        assert bf.host_decode(f)[:2] == (bf.ZH_OK, data), label
        assert _lib.blosc_batch_plan([f], zi.FLAG)[1][0][2] == 1, label
        with pytest.raises(_lib.ZhError) as e:
            _lib.blosc_streams(f, zi.FLAG)
        assert (e.value.status, str(e.value)) == (bf.ZH_EUNSUPPORTED,
                                                  "blosc payload is decoded on the host"), label
    frames, with_flag, without = zi.mixed_batch()
    total, rows = _lib.blosc_batch_plan(frames, zi.FLAG)
    assert [r[2] for r in rows] == with_flag
    assert [r[2] for r in _lib.blosc_batch_plan(frames)[1]] == without
    pos = 0
    for off, nb, _ in rows:
        assert off == pos and off % 256 == 0
        pos = -(-(pos + nb) // 256) * 256
    assert total == pos
    # zlib stays on the host, a memcpyed frame has no streams: as without the flag
    for f in (frames[1], frames[2]):
        with pytest.raises(_lib.ZhError) as e:
            _lib.blosc_streams(f, zi.FLAG)
        assert e.value.status == bf.ZH_EUNSUPPORTED


def test_unknown_flags_are_refused():
    f = zi.matrix()[0][2]
    for call in (lambda: _lib.blosc_batch_plan([f], 2), lambda: _lib.blosc_streams(f, 2),
                 lambda: _lib.blosc_batch_plan([f], 3), lambda: _lib.blosc_batch_plan([], 2)):
        with pytest.raises(_lib.ZhError) as e:
            call()
        assert e.value.status == bf.ZH_EINVAL


def test_corrupt_frames_are_the_host_decoders_to_refuse():
    for label, f, where in zi.corrupt():
        st, _, msg = bf.host_decode(f)
        assert st == bf.ZH_EDATA, label
        if where is None:       # the header check: the plan refuses with the host's words
            with pytest.raises(_lib.ZhError) as e:
                _lib.blosc_batch_plan([f], zi.FLAG)
            assert (e.value.status, str(e.value)) == (st, msg), label
        else:
            assert _lib.blosc_batch_plan([f], zi.FLAG)[1][0][2] == where, label
    texts = {lb: bf.host_decode(f)[2] for lb, f, _ in zi.corrupt()}
    assert texts["truncated by one byte"] == "blosc frame truncated"
    assert texts["flipped sequence bit"] == "corrupt blosc block"
    assert texts["offset before the stream"] == "corrupt blosc block"


# ---- the route's host logic under sanitizers ------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/blosc_zstd_check built with AddressSanitizer + UBSan: a stand-alone host program,
    run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "blosc_zstd_check.cpp")
    exe = str(tmp_path_factory.mktemp("blosc_zstd_check") / "blosc_zstd_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    tried = []
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path is None:
            continue
        for static in (["-static-libasan"], []):  # gcc: the runtime inside the program
            r = subprocess.run([path] + flags + static + ["-o", exe, src], capture_output=True,
                               text=True)
            if r.returncode == 0:
                return exe
            tried.append(f"{path}: {r.stderr[-400:]}")
    pytest.fail("no C++ compiler built the sanitizer checker:\n" + "\n".join(tried))


def test_route_under_sanitizers(checker, tmp_path):
    L = _lib.lib()
    valid = [f for _, _, f in zi.matrix()]
    routed = [f for _, _, f in zi.host_routed()] + zi.mixed_batch()[0]
    bad = [f for _, f, _ in zi.corrupt()]
    frames = valid + routed + bad
    p = tmp_path / "frames.bin"
    with open(p, "wb") as fh:
        for f in frames:
            fh.write(struct.pack("<I", len(f)) + f)
    r = subprocess.run([checker, str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == len(frames)
    streams = 0
    for k, (f, (where, st, h, nz)) in enumerate(zip(frames, lines)):
        where, st, h, nz = int(where), int(st), int(h, 16), int(nz)
        hst, out, _ = bf.host_decode(f)
        try:
            want = _lib.blosc_batch_plan([f], zi.FLAG)[1][0][2]
        except _lib.ZhError:
            want = -1
        # LZ4 / BloscLZ frames are where 0 but not this checker's: it reports what it decodes
        if want == 0 and f[2] >> 5 != 4:
            continue
        assert where == want, k
        if where != 0:
            continue
        assert st == hst, k              # the lane refuses exactly what the host decoder refuses
        if st == bf.ZH_OK:
            assert h == L.zh_xxh64(out, len(out), 0), k
            streams += nz
        if k < len(valid):
            assert st == bf.ZH_OK, k
    assert streams >= len(valid)         # split blocks outnumber the empty frames
    # the corrupt frames planned for the device are refused on the lane
    planned = [ln for ln, (_, _, w) in zip(lines[-len(bad):], zi.corrupt()) if w == 0]
    assert len(planned) >= 3 and all(ln[0] == "0" and ln[1] == str(bf.ZH_EDATA) for ln in planned)
