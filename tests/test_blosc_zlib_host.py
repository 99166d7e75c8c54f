"""The host half of the device decode of blosc frames with zlib streams (ZH_BLOSC_ZLIB_DEVICE:
zh_blosc_batch_plan_ex, zh_debug_blosc_streams_ex, zarr-java_amd/csrc/zh_blosc_streams.h): the
plan and the stream table with and without the flag, and the route's host-side logic (plan, rows,
the zlib stream reader and its Adler-32 on one lane, the unshuffle) against zlib's uncompress under
AddressSanitizer + UBSan in a stand-alone program over the valid matrix, the corrupt frames and
seeded mutations.  No GPU."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import blosc_frames as bf
import blosc_zlib_inputs as li
from zarrhip import _abi as A
from zarrhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan and the stream table ----------------------------------------------------------------
def test_matrix_is_planned_for_the_device_only_with_the_flag():
    assert A.ZH_BLOSC_ZLIB_DEVICE == li.FLAG
    for label, data, f in li.matrix():
        st, out, msg = bf.host_decode(f)
        assert (st, out) == (bf.ZH_OK, data), (label, msg)
        total, rows = _lib.blosc_batch_plan([f], li.FLAG)
        assert rows == [(0, len(data), 0)] and total == -(-len(data) // 256) * 256, label
        for flags in (0, li.ZSTD_FLAG):
            assert _lib.blosc_batch_plan([f], flags) == (total, [(0, len(data), 1)]), label
        assert _lib.blosc_batch_plan([f]) == (total, [(0, len(data), 1)]), label
        # without the flag the table refuses the frame exactly as it always has
        for call in (lambda: _lib.blosc_streams(f), lambda: _lib.blosc_streams(f, li.ZSTD_FLAG)):
            with pytest.raises(_lib.ZhError) as e:
                call()
            assert (e.value.status, str(e.value)) == (bf.ZH_EUNSUPPORTED,
                                                      "blosc payload is decoded on the host"), label


def walk(f):
    """The block / stream rows of a zlib frame by a walk written here."""
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
            rows.append((1, pos, cs, s * want, want, 0 if cs == want else li.KZLIB))
            pos += cs
    return rows


def test_stream_table_with_the_flag():
    seen = set()
    for label, data, f in li.matrix():
        rows = _lib.blosc_streams(f, li.FLAG)
        assert rows == walk(f), label
        assert rows == _lib.blosc_streams(f, li.FLAG | li.ZSTD_FLAG), label
        for r in rows:
            seen.add(("block", r[4], r[5], r[2] > li.LDS_BLOCK) if r[0] == 0 else ("stream", r[5]))
    blocks = {k[1:] for k in seen if k[0] == "block"}
    assert {k[1] for k in seen if k[0] == "stream"} == {0, li.KZLIB}
    assert {b[0] for b in blocks} == {0, 1, 2, 3}            # every shuffle kind
    assert {b[1] for b in blocks} == {1, 4, 8}               # unsplit, 4 and 8 streams
    assert (1, 1, True) in blocks and (0, 1, True) in blocks  # blocks beyond the LDS window
    # the split block of `quad`: a raw stream, then three zlib streams
    f = next(f for lb, _, f in li.matrix() if lb.startswith("split, raw and constant"))
    assert [r[5] for r in _lib.blosc_streams(f, li.FLAG) if r[0] == 1] == [0, 4, 4, 4]
    # LZ4 / BloscLZ frames: the same table with the flag as without
    for label, f in bf.matrix()[::17]:
        assert _lib.blosc_streams(f, li.FLAG) == _lib.blosc_streams(f), label


def block_types(stream):
    """The BTYPEs of a zlib stream's DEFLATE blocks, by the library's gzip block diagnostic on
    the same blocks in a gzip member."""
    d = zlib.decompressobj()
    body = d.decompress(stream)
    raw = stream[2:len(stream) - len(d.unused_data) - 4]
    member = b"\x1f\x8b\x08\x00" + bytes(6) + raw + struct.pack("<II", zlib.crc32(body), len(body))
    return [r[0] for r in _lib.gzip_blocks(member)]


def test_matrix_covers_the_block_kinds():
    """The inputs cannot silently stop reaching stored, fixed and dynamic blocks, an empty stored
    block between compressed ones, and a stream of several blocks."""
    kinds = {}
    for label, data, f in li.matrix():
        for s in li.zlib_streams(f):
            kinds[label] = kinds.get(label, []) + block_types(s)
    assert set(kinds["level 0: stored blocks"]) == {0}
    assert set(kinds["Z_FIXED"]) == {1}
    assert 2 in kinds["level 6"] and 2 in kinds["Z_RLE"] and 2 in kinds["Z_HUFFMAN_ONLY"]
    assert kinds["sync flush in the middle"][1] == 0 and len(kinds["sync flush in the middle"]) >= 3
    assert len(kinds["160 KiB in one stream"]) > 1
    assert kinds["matches at distance 32768"] == [0, 1]


def test_host_routed_and_mixed_frames():
    for label, data, f in li.host_routed():
        assert bf.host_decode(f)[:2] == (bf.ZH_OK, data), label
        assert _lib.blosc_batch_plan([f], li.FLAG)[1][0][2] == 1, label
        with pytest.raises(_lib.ZhError) as e:
            _lib.blosc_streams(f, li.FLAG)
        assert (e.value.status, str(e.value)) == (bf.ZH_EUNSUPPORTED,
                                                  "blosc payload is decoded on the host"), label
    frames, wheres = li.mixed_batch()
    assert wheres[5] == [0, 2, 0, 0]
    for flags, want in wheres.items():
        total, rows = _lib.blosc_batch_plan(frames, flags)
        assert [r[2] for r in rows] == want, flags
        pos = 0
        for off, nb, _ in rows:
            assert off == pos and off % 256 == 0
            pos = -(-(pos + nb) // 256) * 256
        assert total == pos
    # a memcpyed frame has no streams, with any flag
    with pytest.raises(_lib.ZhError) as e:
        _lib.blosc_streams(frames[1], li.FLAG)
    assert e.value.status == bf.ZH_EUNSUPPORTED


def test_unknown_flags_are_refused():
    f = li.matrix()[0][2]
    for flags in (2, 3, 6, 7, 8):
        for call in (lambda: _lib.blosc_batch_plan([f], flags),
                     lambda: _lib.blosc_streams(f, flags),
                     lambda: _lib.blosc_batch_plan([], flags)):
            with pytest.raises(_lib.ZhError) as e:
                call()
            assert e.value.status == bf.ZH_EINVAL, flags


def test_corrupt_frames_are_the_host_decoders_to_refuse():
    for label, f, where in li.corrupt():
        st, _, msg = bf.host_decode(f)
        assert st == bf.ZH_EDATA, label
        assert _lib.blosc_batch_plan([f], li.FLAG)[1][0][2] == where, label
    texts = {lb: bf.host_decode(f)[2] for lb, f, _ in li.corrupt()}
    assert texts.pop("truncated by one byte") == "blosc frame truncated"
    assert set(texts.values()) == {"corrupt blosc block"}


# ---- the route's host logic under sanitizers ------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/blosc_zlib_check built with AddressSanitizer + UBSan: a stand-alone host program,
    run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "blosc_zlib_check.cpp")
    exe = str(tmp_path_factory.mktemp("blosc_zlib_check") / "blosc_zlib_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    tried = []
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path is None:
            continue
        for static in (["-static-libasan"], []):  # gcc: the runtime inside the program
            r = subprocess.run([path] + flags + static + ["-o", exe, src, "-lz"],
                               capture_output=True, text=True)
            if r.returncode == 0:
                return exe
            tried.append(f"{path}: {r.stderr[-400:]}")
    pytest.fail("no C++ compiler built the sanitizer checker:\n" + "\n".join(tried))


def run_checker(checker, path, frames, *args):
    with open(path, "wb") as fh:
        for f in frames:
            fh.write(struct.pack("<I", len(f)) + f)
    r = subprocess.run([checker, str(path)] + [str(a) for a in args], capture_output=True,
                       text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == len(frames) + 1 and lines[-1][0] == "mutations"
    return lines[:-1], int(lines[-1][1])


def test_route_under_sanitizers(checker, tmp_path):
    """Every stream of every frame: decode_zlib_stream and adler32 on one lane accept and reject
    with uncompress and give its bytes (the checker's exit status); every frame the plan admits:
    decode_frame_serial with the flag is zh_blosc_decompress."""
    L = _lib.lib()
    valid = [f for _, _, f in li.matrix()]
    routed = [f for _, _, f in li.host_routed()] + li.mixed_batch()[0]
    bad = [f for _, f, _ in li.corrupt()]
    frames = valid + routed + bad
    lines, _ = run_checker(checker, tmp_path / "frames.bin", frames)
    judged = 0
    for k, (f, (where, st, h, ns)) in enumerate(zip(frames, lines)):
        where, st, h, ns = int(where), int(st), int(h, 16), int(ns)
        hst, out, _ = bf.host_decode(f)
        want = _lib.blosc_batch_plan([f], li.FLAG)[1][0][2]
        # LZ4 / BloscLZ frames are where 0 but not this checker's: it reports what it decodes
        if f[2] >> 5 != 3:
            continue
        assert where == want, k
        judged += ns
        if where != 0:
            continue
        assert st == hst, k              # the lane refuses exactly what the host decoder refuses
        if st == bf.ZH_OK:
            assert h == L.zh_xxh64(out, len(out), 0), k
        if k < len(valid):
            assert st == bf.ZH_OK, k
    assert judged >= len(frames) - 5     # split blocks outnumber the empty and the foreign frames
    # the corrupt frames planned for the device are refused on the lane
    planned = [ln for ln, (_, _, w) in zip(lines[-len(bad):], li.corrupt()) if w == 0]
    assert len(planned) == 6 and all(ln[0] == "0" and ln[1] == str(bf.ZH_EDATA) for ln in planned)


def test_mutated_streams_under_sanitizers(checker, tmp_path):
    """A few thousand seeded single-byte and single-bit mutations of the matrix streams: the lane
    and uncompress agree on every one (the checker's exit status)."""
    frames = li.mutation_inputs()
    _, n = run_checker(checker, tmp_path / "mutate.bin", frames, 60, 20250114)
    assert n >= 3000
