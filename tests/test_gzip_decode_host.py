"""The gzip member decoder on the host (zh_gzip_decompress, zh_gzip_batch_plan,
zh_debug_gzip_blocks; zarr-java_amd/csrc/zh_gzip_dec.h run on one lane).  zlib is the reference:
GzipCodec.decode is zlib.decompress(b, 31), so the decoder has to accept and reject exactly what
zlib accepts and rejects.  No device."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import gzip_dec_inputs as gi
from helpers import ROOT
from zarrhip import _abi as A
from zarrhip import _lib

N_MUTATIONS = 1200


def test_inputs_reach_the_cases_they_are_meant_to():
    cov = gi.coverage()
    assert cov["fifteen_bit_code"]
    assert cov["one_distance_code"] and cov["no_distance_code"]
    assert cov["distance_32768"]
    assert cov["block_types"] == {0, 1, 2}
    assert cov["several_dynamic_blocks"]
    # the Fibonacci member uses the code-length symbols 17 and 18 (zero runs between its 23
    # literals) and has 15-bit literal codes
    fib = [m for label, _, m in gi.valid() if label == "fibonacci counts"][0]
    assert max(r[5] for r in _lib.gzip_blocks(fib)) == 15
    rows = _lib.gzip_blocks([m for label, _, m in gi.valid() if label == "mixed blocks"][0])
    assert [r[0] for r in rows] == [2, 1, 0, 2]
    assert sum(r[2] for r in rows) == 33 and all(r[1] > 0 for r in rows)


def test_valid_set_equals_zlib():
    for label, data, m in gi.valid():
        assert _lib.gzip_decompress(m) == data, label
        assert zlib.decompress(m, 31) == data, label
        assert _lib.gzip_size(m) == len(data), label
    for label, data, m, _ in gi.host_routed():
        assert _lib.gzip_decompress(m) == data == zlib.decompress(m, 31), label
        assert _lib.gzip_size(m) == len(data), label


def test_corrupt_members_have_their_text():
    kinds = [k for k, _ in gi.corrupt()]
    assert set(kinds) == set(gi.TEXTS) and len(kinds) == len(set(kinds)) == 20
    for kind, m in gi.corrupt():
        st, _, msg = gi.host_decode(m)
        assert (st, msg) == (A.ZH_EDATA, gi.TEXTS[kind]), kind
        if kind != "CRC mismatch":     # the size query does not hash
            with pytest.raises(_lib.ZhError) as e:
                _lib.gzip_size(m)
            assert str(e.value) == msg, kind
    # room: content larger than dstcap is the caller's error, not the member's
    import ctypes as C
    m = gi.valid()[1][2]
    n = C.c_size_t()
    err = C.create_string_buffer(256)
    out = C.create_string_buffer(100)
    st = _lib.lib().zh_gzip_decompress(m, len(m), out, 100, C.byref(n), err, 256)
    assert (st, err.value) == (A.ZH_EINVAL, b"gzip: decoded data exceeds the output buffer")


def test_mutations_agree_with_zlib():
    """Seeded mutations of the small members: both reject, or both accept with equal bytes.  No
    share may disagree: zlib is the host route, so another accept set would change what reads
    succeed."""
    accepted = rejected = 0
    for k, m in enumerate(gi.mutations(N_MUTATIONS)):
        try:
            want = zlib.decompress(m, 31)
        except zlib.error:
            want = None
        st, got, msg = gi.host_decode(m)
        assert (got is None) == (want is None), (k, m.hex(), msg)
        assert got == want, (k, m.hex())
        accepted += want is not None
        rejected += want is None
    print(f"{accepted} mutations accepted by both, {rejected} rejected by both")
    assert accepted >= 20 and rejected >= 600       # the set exercises both sides


def test_plan():
    valid = gi.valid()
    total, rows = _lib.gzip_batch_plan([m for _, _, m in valid])
    pos = 0
    for (label, data, _), (off, nb, where) in zip(valid, rows):
        assert (off, nb, where) == (pos, len(data), 0), label
        assert off % 256 == 0
        pos = -(-(pos + nb) // 256) * 256
    assert total == pos
    assert _lib.gzip_batch_plan([]) == (0, [])
    # The frames the plan itself sends to the host.  The plan walks the header only: trailing
    # bytes and host_only show in it; a second member does not (its size could be the first
    # one's: DEFLATE's 1032-fold bound holds for the pair as well), so that frame is planned
    # for the device with the second member's size, its wave refuses it (the member does not end
    # with the frame) and the batch call hands it to the host: test_gpu_gzip_decode.py.
    routed = gi.host_routed()
    frames, keep = gi.frames_of(routed)
    _, rows = _lib.gzip_batch_plan(frames)
    by = {label: (nb, where) for (label, *_), (_, nb, where) in zip(routed, rows)}
    assert by["trailing bytes"] == (len(routed[0][1]), 1)
    assert by["host_only"] == (len(routed[2][1]), 1)
    assert by["two members"][0] == struct.unpack("<I", routed[1][2][-4:])[0]
    assert by["hidden size"] == (1, 0)
    # too short behind the header for a block and a trailer: the size query judges it
    with pytest.raises(_lib.ZhError) as e:
        _lib.gzip_batch_plan([gi.HEADER + b"\x03\x00" + bytes(7)])
    assert str(e.value) == "gzip: trailer truncated"
    # a header error is the first bad frame's in batch order, with the host text
    bad = dict(gi.corrupt())
    good = valid[1][2]
    for first, second in (("magic", "FHCRC mismatch"), ("FHCRC mismatch", "magic"),
                          ("reserved FLG bit", "CM")):
        with pytest.raises(_lib.ZhError) as e:
            _lib.gzip_batch_plan([good, bad[first], good, bad[second]])
        assert (e.value.status, str(e.value)) == (A.ZH_EDATA, gi.TEXTS[first])
    # a stream error does not show in the plan: the header alone is walked
    _, rows = _lib.gzip_batch_plan([good, bad["distance too far back"]])
    assert [w for _, _, w in rows] == [0, 0]


# ---- the decoder under sanitizers ----------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/gzip_dec_check built with AddressSanitizer + UBSan, as test_gzip_encode_host.py
    builds gzip_enc_check: stand-alone, run directly."""
    src = os.path.join(ROOT, "zarr-java_amd", "tools", "gzip_dec_check.cpp")
    exe = str(tmp_path_factory.mktemp("gzip_dec_check") / "gzip_dec_check")
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


def test_decoder_under_sanitizers(checker, tmp_path):
    members = ([m for _, _, m in gi.valid()] + [m for _, _, m, _ in gi.host_routed()] +
               [m for _, m in gi.corrupt()] + gi.mutations(N_MUTATIONS))
    path = tmp_path / "members.bin"
    with open(path, "wb") as fh:
        for m in members:
            fh.write(struct.pack("<I", len(m)) + m)
    r = subprocess.run([checker, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(members) and all(ln.endswith(" ok") for ln in lines)
    n_valid = len(gi.valid())
    for (label, data, _), ln in zip(gi.valid(), lines):
        assert ln == f"0 0 {len(data)} ok", label     # the kernel's call ran on every valid member
    assert all(ln.split()[1] != "0" or ln.split()[2] == "0"
               for ln in lines[n_valid + 4:n_valid + 4 + 20])   # corrupt(): none accepted
