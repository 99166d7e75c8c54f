"""The gzip member writer with dynamic-Huffman segments on the host (zh_gzip_compress with
zh_gzip_enc_params::dynamic = 1; zarr-java_amd/csrc/zh_gzip_enc.h): every member of the matrix
decodes with zlib, Python's gzip and the library's own reader; no member grows; dynamic = 0 is
the writer of before; the header of every dynamic segment follows the stated rules and the
segment is strictly the smallest form; the code lengths (zh_debug_gzip_code_lengths) are
length-limited, complete and optimal where the limit allows; sizes against zlib; and the writer
under AddressSanitizer + UBSan in a stand-alone program.  No GPU."""
import ctypes as C
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import gzip_dyn_inputs as gd
import gzip_enc_inputs as gi
from zarrhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = gd.matrix()


@pytest.fixture(scope="module")
def members():
    return [_lib.gzip_compress(d, bs, dynamic=True) for _, d, bs in MATRIX]


@pytest.fixture(scope="module")
def walked(members):
    return {r[0]: gd.segments(f) for r, f in zip(MATRIX, members)}


def test_members_decode_to_their_input(members):
    for (label, data, bs), f in zip(MATRIX, members):
        assert zlib.decompress(f, 31) == data, label
        assert gzip.decompress(f) == data, label
        assert _lib.gzip_decompress(f) == data, label
        assert f[:10] == gi.HEADER, label
        assert f[-10:-8] == b"\x03\x00", label
        assert struct.unpack("<II", f[-8:]) == (zlib.crc32(data), len(data) % 2 ** 32), label
        assert f == _lib.gzip_compress(data, bs, dynamic=True), label     # twice: the same bytes


def test_never_larger_and_the_bound(members):
    L = _lib.lib()
    for (label, data, bs), f in zip(MATRIX, members):
        before = _lib.gzip_compress(data, bs)
        assert len(f) <= len(before), label
        assert _lib.gzip_compress(data, bs, dynamic=False) == before, label
        prm = _lib.A.zh_gzip_enc_params(bs, 1)
        n = C.c_size_t()
        assert L.zh_gzip_compress(data, len(data), C.byref(prm), None, 0, C.byref(n), None, 0) == 0
        assert n.value == gi.bound(len(data), bs) and len(f) <= n.value, label


def test_params():
    L = _lib.lib()
    n = C.c_size_t()
    err = C.create_string_buffer(256)
    for bad in (2, -1):
        prm = _lib.A.zh_gzip_enc_params(0, bad)
        assert L.zh_gzip_compress(b"abc", 3, C.byref(prm), None, 0, C.byref(n), err,
                                  256) == _lib.A.ZH_EINVAL
        assert err.value == b"zh_gzip_compress: dynamic is 0 or 1"
    prm = _lib.A.zh_gzip_enc_params(-1, 1)
    assert L.zh_gzip_compress(b"abc", 3, C.byref(prm), None, 0, C.byref(n), err,
                              256) == _lib.A.ZH_EINVAL
    assert err.value == b"zh_gzip_compress: blocksize >= 0"
    assert C.sizeof(_lib.A.zh_gzip_enc_params) == 8
    assert _lib.A.zh_gzip_enc_params(7).dynamic == 0          # one argument: the writer of before


def test_coverage(walked):
    """What the matrix reaches."""
    forms = lambda label: [s["form"] for s in walked[label]]  # noqa: E731
    every = [s for segs in walked.values() for s in segs]
    assert {s["form"] for s in every} == {"stored", "fixed", "dynamic"}
    assert forms("mix-b0") == ["stored", "dynamic"]           # noise, then noise and zeros
    for label, segs in walked.items():
        if label.startswith("random-"):
            assert {s["form"] for s in segs} <= {"stored"}, label
    dyn = [s for s in every if s["form"] == "dynamic"]
    sent = {sym for s in dyn for sym, _ in s["cl_syms"]}
    assert {16, 17, 18} <= sent
    used = lambda s: sum(1 for n in s["d_lens"] if n)         # noqa: E731
    assert any(used(s) == 0 for s in dyn) and any(used(s) == 1 for s in dyn)
    assert any(used(s) > 1 for s in dyn)
    assert any(s["hlit"] == 257 for s in dyn) and any(s["hlit"] > 257 for s in dyn)
    assert any(s["hlit"] == 286 for s in dyn)                 # a piece of 258 bytes: code 285
    assert {s["form"] for s in walked["noisy-b0"]} == {"dynamic"}
    assert {s["form"] for s in walked["pattern3-b0"]} == {"dynamic"}
    assert all(used(s) == 1 for s in walked["pattern3-b0"])   # every match at distance 3
    assert forms("short-b0") == ["stored"] and forms("all_values-b0") == ["stored"]
    assert {s["form"] for s in walked["high_bytes-b0"]} == {"dynamic"}    # stored before
    assert all(used(s) == 0 and s["hdist"] == 1 and s["hlit"] == 257
               for s in walked["high_bytes-b0"])


def test_dynamic_segments_follow_the_rules(walked):
    n = 0
    for label, segs in walked.items():
        for s in segs:
            if s["form"] != "dynamic":
                continue
            n += 1
            hist, ll, dl = s["hist"], s["ll_lens"], s["d_lens"]
            # the sets: exactly the used symbols have a code; complete, or the two exceptions
            assert [c > 0 for c in hist] == [v > 0 for v in ll + dl], label
            assert max(ll + dl) <= 15 and hist[256] == 1, label
            assert gd.kraft(ll) == 1 << 15, label
            nd = sum(1 for v in dl if v)
            if nd == 0:
                assert s["hdist"] == 1 and dl[0] == 0, label
            elif nd == 1:
                assert max(dl) == 1, label
            else:
                assert gd.kraft(dl) == 1 << 15, label
            # the optimal cost where the limit allows, and no longer code for a larger count
            for counts, lens in ((hist[:gd.LITLEN], ll), (hist[gd.LITLEN:], dl)):
                if sum(1 for c in counts if c) < 2:
                    continue
                cost, depth = gd.huffman_cost(counts)
                assert depth <= 15, label                     # see test_code_lengths
                assert sum(c * v for c, v in zip(counts, lens)) == cost, label
                order = sorted((c, v) for c, v in zip(counts, lens) if c)
                assert all(a[1] >= b[1] for a, b in zip(order, order[1:]) if a[0] < b[0]), label
            # the header: trimmed counts, the greedy run-length coding, the code-length code
            assert s["hlit"] == max(257, max(k + 1 for k, v in enumerate(ll) if v)), label
            assert s["hdist"] == max([1] + [k + 1 for k, v in enumerate(dl) if v]), label
            assert s["cl_syms"] == gd.rle(ll[:s["hlit"]] + dl[:s["hdist"]]), label
            cl = s["cl_lens"]
            clhist = [sum(1 for sym, _ in s["cl_syms"] if sym == k) for k in range(19)]
            assert [c > 0 for c in clhist] == [v > 0 for v in cl], label
            assert max(cl) <= 7 and sum(1 << (7 - v) for v in cl if v) == 1 << 7, label
            cost, depth = gd.huffman_cost(clhist)
            got = sum(c * v for c, v in zip(clhist, cl))
            assert got == cost if depth <= 7 else got >= cost, label
            assert s["hclen"] == max(4, max(k + 1 for k, o in enumerate(gd.CL_ORDER) if cl[o])), \
                label
            # the choice: strictly the smallest, from the sizes the histogram gives
            assert s["bytes"] == s["dyn_bytes"], label
            assert s["bytes"] < s["fixed_bytes"] and s["bytes"] < s["stored_bytes"], label
    assert n > 100


def test_segments_one_byte_under_stored():
    """The last size at which a dynamic segment is still chosen, at each place of its
    end-of-block code in the byte before the marker."""
    seen = set()
    for label, data, bs, bits in gd.edge_rows():
        f = _lib.gzip_compress(data, bs, dynamic=True)
        assert zlib.decompress(f, 31) == data and _lib.gzip_decompress(f) == data, label
        (s,) = gd.segments(f)
        assert s["form"] == "dynamic" and s["bytes"] == len(data) + 4 == s["stored_bytes"] - 1
        assert s["bits"] == bits and 8 * len(data) - 9 <= bits <= 8 * len(data) - 3, label
        seen.add(bits % 8)
    assert len(seen) == 7


def test_other_segments_are_the_choice_of_before(walked):
    """A fixed segment is smaller than stored and a stored one not larger than fixed, as before;
    and the sizes the reader recomputes are the sizes on the page."""
    for label, segs in walked.items():
        for s in segs:
            if s["form"] == "fixed":
                assert s["bytes"] == s["fixed_bytes"] < s["stored_bytes"], label
    # without a dynamic segment in it, a member is the member of before
    for (label, data, bs) in MATRIX:
        if all(s["form"] != "dynamic" for s in walked[label]):
            assert _lib.gzip_compress(data, bs, dynamic=True) == _lib.gzip_compress(data, bs), label


# ---- the code lengths ---------------------------------------------------------------------------
def check_code_lengths(label, limit, rows, out):
    assert len(out) == len(rows), label
    for counts, lens in zip(rows, out):
        used = sum(1 for c in counts if c)
        assert [c > 0 for c in counts] == [v > 0 for v in lens], label
        if used == 0:
            continue
        if used == 1:
            assert max(lens) == 1, label
            continue
        assert max(lens) <= limit, label
        assert sum(1 << (limit - v) for v in lens if v) == 1 << limit, label
        cost, depth = gd.huffman_cost(counts)
        got = sum(c * v for c, v in zip(counts, lens))
        if depth <= limit:
            assert got == cost, (label, got, cost)
        else:
            assert got >= cost, (label, got, cost)            # a bound for any limited code
        order = sorted((c, v) for c, v in zip(counts, lens) if c)
        assert all(a[1] >= b[1] for a, b in zip(order, order[1:]) if a[0] < b[0]), label


def test_code_lengths():
    """The matcher flattens skewed inputs (the shuffled Fibonacci block below has a depth of 14
    after matching), so no end-to-end input reaches the limit of 15 bits: the unit entry does."""
    limited = 0
    for label, nsym, limit, rows in gd.histogram_sets():
        out = _lib.gzip_code_lengths(rows, limit)
        check_code_lengths(label, limit, rows, out)
        assert out == _lib.gzip_code_lengths(rows, limit), label
        limited += sum(1 for r in rows if sum(1 for c in r if c) > 1
                       and gd.huffman_cost(r)[1] > limit)
        if label.startswith("fibonacci"):
            assert all(max(v) == limit for v in out), label
    assert limited > 30
    # two symbols, one symbol
    assert _lib.gzip_code_lengths([[0, 9, 0, 2]], 15) == [[0, 1, 0, 1]]
    assert _lib.gzip_code_lengths([[0, 0, 4, 0]], 15) == [[0, 0, 1, 0]]
    # ties: of equally frequent symbols the lower has the longer code
    assert _lib.gzip_code_lengths([[1, 1, 1]], 15) == [[2, 2, 1]]
    L = _lib.lib()
    lens = (C.c_uint8 * 4)()
    counts = (C.c_uint32 * 4)(1, 2, 3, 4)
    for nsym, limit in ((0, 15), (287, 15), (4, 0), (4, 16)):
        assert L.zh_debug_gzip_code_lengths(None, counts, nsym, limit, 1, lens) == \
            _lib.A.ZH_EINVAL
    assert L.zh_debug_gzip_code_lengths(None, (C.c_uint32 * 4)(1, 1, 1, 1), 4, 1, 1, lens) == \
        _lib.A.ZH_EINVAL                                      # four symbols, one bit: no code


def test_fibonacci_block_stays_under_the_limit():
    rng = np.random.default_rng(31)
    fib = gd.fibonacci(21)                                    # 28 656 bytes
    data = np.repeat(np.arange(21, dtype=np.uint8) + 65, fib)
    assert len(data) == 28656
    rng.shuffle(data)
    data = data.tobytes()
    assert gd.huffman_cost(fib)[1] == 20                      # before matching
    f = _lib.gzip_compress(data, gi.MAX_BLOCK, dynamic=True)
    assert zlib.decompress(f, 31) == data
    (seg,) = gd.segments(f)
    assert seg["form"] == "dynamic"
    depth = gd.huffman_cost(seg["hist"][:gd.LITLEN])[1]
    print(f"depth after matching: {depth}")
    assert depth == max(seg["ll_lens"]) <= 15


# ---- sizes --------------------------------------------------------------------------------------
def test_sizes_against_zlib():
    """Member bytes at the default block size with dynamic segments against the writer of before
    and zlib levels 1 and 5 on the same bytes.  Measured (the table of DESIGN.md,
    "Dynamic-Huffman segments"):
      labels   262 144 B:   8 664 B before,   6 136 B dynamic; zlib level 1   4 964 B (1.2361),
               level 5   6 260 B (0.9802)
      text      69 237 B:  24 085 B before,  14 736 B dynamic; zlib level 1  14 278 B (1.0321),
               level 5  10 467 B (1.4079)
      zeros    262 144 B:   1 812 B before,     612 B dynamic; zlib level 1   1 179 B (0.5191),
               level 5     289 B (2.1176)
      noisy    262 144 B: 262 244 B before, 216 087 B dynamic; zlib level 1 195 961 B (1.1027),
               level 5 195 237 B (1.1068)
    Asserted on labels, text and noisy: the measured worst ratio to zlib level 1, 1.2361, plus
    0.10, the headroom the writer's test of before leaves for a later retune of the hash.  The
    noisy image holds no stored segment any more and is smaller than raw."""
    worst = 0.0
    for name, data in (("labels", gi.labels()), ("text", gi.text()), ("zeros", bytes(1 << 18)),
                       ("noisy", gd.noisy())):
        before = len(_lib.gzip_compress(data))
        f = _lib.gzip_compress(data, dynamic=True)
        ours = len(f)
        z1, z5 = len(gzip.compress(data, 1, mtime=0)), len(gzip.compress(data, 5, mtime=0))
        print(f"{name}: raw {len(data)} B, zh_gzip_compress {before} B, dynamic {ours} B, "
              f"zlib level 1 {z1} B (ratio {ours / z1:.4f}), zlib level 5 {z5} B "
              f"(ratio {ours / z5:.4f})")
        if name != "zeros":
            worst = max(worst, ours / z1)
            assert ours <= z1 * 1.3361, (name, ours, z1)
        if name == "noisy":
            rows = _lib.gzip_blocks(f)            # (type, stored bits, decoded bytes, ...)
            assert rows[-1][0] == 1 and rows[-1][2] == 0              # the ending 03 00
            assert [r[0] for r in rows[:-1]] == [2, 0] * 16           # dynamic, then its marker
            assert all(r[2] == 0 for r in rows if r[0] == 0)          # nothing is stored
            assert ours < len(data)
    print(f"worst ratio to zlib level 1 on labels, text and noisy: {worst:.4f}")


# ---- the writer under sanitizers ----------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/gzip_enc_check built with AddressSanitizer + UBSan, as test_gzip_encode_host.py
    builds it: stand-alone, run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "gzip_enc_check.cpp")
    exe = str(tmp_path_factory.mktemp("gzip_enc_check") / "gzip_enc_check")
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


def test_writer_under_sanitizers(checker, members, tmp_path):
    src, dst = tmp_path / "buffers.bin", tmp_path / "members.bin"
    with open(src, "wb") as fh:
        for _, data, bs in MATRIX:
            fh.write(struct.pack("<II", len(data), bs) + data)
    r = subprocess.run([checker, str(src), str(dst), "1"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(MATRIX) and all(ln.endswith(" ok") for ln in lines)
    raw = open(dst, "rb").read()
    pos = 0
    for (label, *_), f in zip(MATRIX, members):
        (n,) = struct.unpack("<I", raw[pos:pos + 4])
        assert raw[pos + 4:pos + 4 + n] == f, label   # the library's build gives the same bytes
        pos += 4 + n
    assert pos == len(raw)
    r = subprocess.run([checker, str(src), str(dst), "2"], capture_output=True, text=True)
    assert not r.stderr and all(ln.startswith("1 0 ") for ln in r.stdout.splitlines())
