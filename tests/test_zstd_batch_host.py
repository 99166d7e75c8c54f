"""The host half of the batched device zstd decode (zarr-java_amd/csrc/zh_zstd_dec.h,
zh_zstd_batch_plan, zh_debug_zstd_blocks): the batch plan against zh_zstd_decompress's size query,
the block table against a walk written here, and the shared decoder's serial form under
AddressSanitizer + UBSan in a stand-alone program over valid, mutated and corrupt frames.  No
GPU."""
import os
import shutil
import struct
import subprocess

import pytest

import zstd_dec_inputs as zi
from zarrhip import _abi as A
from zarrhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_built_frames_decode_with_libzstd():
    """A hand-built frame that libzstd rejects is a bug of the helper, not of a decoder."""
    for label, data, frame in zi.valid():
        if label.startswith("hand") or label.startswith("empty"):
            zi.check_with_libzstd(data, frame)
    for label, data, frame in zi.host_routed():
        if label != "concatenated":      # pyarrow decodes one frame into an exact buffer
            continue
        assert zi.host_decode(frame)[1] == data


# ---- the plan ----------------------------------------------------------------------------------
def test_plan_matches_the_size_query():
    frames = [f for _, _, f in zi.valid()]
    total, rows = _lib.zstd_batch_plan(frames)
    pos = 0
    for (label, data, f), (off, nb, where) in zip(zi.valid(), rows):
        st, want, _ = zi.size_query(f)
        assert st == A.ZH_OK and nb == want == len(data), label
        assert off == pos and off % 256 == 0, label
        assert where == 0, label
        pos = -(-(pos + nb) // 256) * 256
    assert total == pos


def test_plan_sends_what_is_not_one_plain_frame_to_the_host():
    routed = zi.host_routed()
    _, rows = _lib.zstd_batch_plan([f for _, _, f in routed] + [zi.impossible_size()])
    assert [r[2] for r in rows] == [1] * (len(routed) + 1)
    for (label, data, f), (_, nb, _) in zip(routed, rows):
        assert nb == len(data) == zi.size_query(f)[1], label
    assert rows[-1][1] == 11
    # a chain that does not end at the last byte, and a truncated block: the host decides
    good = zi.valid()[0][2]
    for f in (good + b"\0", good[:-3]):
        st, nb, msg = zi.size_query(f)
        if st == A.ZH_OK:
            assert _lib.zstd_batch_plan([f])[1][0][2] == 1
        else:
            with pytest.raises(_lib.ZhError) as e:
                _lib.zstd_batch_plan([f])
            assert (e.value.status, str(e.value)) == (st, msg)


def test_plan_reports_the_size_query_failure_first_in_batch_order():
    good = zi.valid()[0][2]
    bad_magic = b"\x27" + good[1:]
    cases = [bad_magic, b"", good[:3], good[:5], b"\x28\xb5\x2f\xfd\x08" + good[5:]]
    for f in cases:
        st, _, msg = zi.size_query(f)
        assert st != A.ZH_OK
        with pytest.raises(_lib.ZhError) as e:
            _lib.zstd_batch_plan([good, f, bad_magic])
        assert (e.value.status, str(e.value)) == (st, msg)
    assert zi.size_query(bad_magic)[2] == "zstd: unknown frame magic"
    # every mutated frame: the same verdict as the size query
    for f in zi.mutations(300, seed=5):
        st, nb, msg = zi.size_query(f)
        try:
            got = (A.ZH_OK, _lib.zstd_batch_plan([f])[1][0][1], "")
        except _lib.ZhError as e:
            got = (e.status, 0, str(e))
        assert got == (st, nb if st == A.ZH_OK else 0, msg if st != A.ZH_OK else "")


# ---- the block table ---------------------------------------------------------------------------
def test_block_table_matches_an_independent_walk():
    seen = {"block": set(), "lit": set(), "streams": set(), "count": set(),
            "ll": set(), "of": set(), "ml": set()}
    for label, _, f in zi.valid():
        rows = _lib.zstd_blocks(f)
        assert rows == zi.independent_blocks(f), label
        for r in rows:
            seen["block"].add(r[0])
            if r[0] != 2:
                continue
            seen["lit"].add(r[3])
            seen["streams"].add(r[4])
            seen["count"].add(0 if r[6] == 0 else 1 if r[6] < 128 else 2 if r[6] < 0x7F00 else 3)
            if r[6]:
                seen["ll"].add(r[7]), seen["of"].add(r[8]), seen["ml"].add(r[9])
    # the inputs reach what they are there for; a later change cannot silently lose a case
    assert seen["block"] == {0, 1, 2}
    assert seen["lit"] == {0, 1, 2, 3}
    assert seen["streams"] >= {1, 4}
    assert seen["count"] == {0, 1, 2, 3}
    assert seen["ll"] == {0, 1, 2, 3} and seen["of"] == {0, 1, 2, 3} and \
        seen["ml"] == {0, 1, 2, 3}


def test_block_table_refuses_host_routed_frames():
    for _, _, f in zi.host_routed():
        with pytest.raises(_lib.ZhError) as e:
            _lib.zstd_blocks(f)
        assert e.value.status == A.ZH_EUNSUPPORTED


# ---- the shared decoder under sanitizers -----------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/zstd_dec_check built with AddressSanitizer + UBSan: a stand-alone host program, run
    directly."""
    srcs = [os.path.join(ROOT, "zarr-java_amd", "tools", "zstd_dec_check.cpp"),
            os.path.join(ROOT, "zarr-java_amd", "csrc", "zh_zstd.cpp")]
    exe = str(tmp_path_factory.mktemp("zstd_check") / "zstd_dec_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    tried = []
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path is None:
            continue
        for static in (["-static-libasan"], []):  # gcc: the runtime inside the program
            r = subprocess.run([path] + flags + static + ["-o", exe] + srcs, capture_output=True,
                               text=True)
            if r.returncode == 0:
                return exe
            tried.append(f"{path}: {r.stderr[-400:]}")
    pytest.skip("no C++ compiler here links the sanitizer runtime into the checker:\n" +
                "\n".join(tried))


def run_checker(exe, frames, tmp_path):
    p = tmp_path / "frames.bin"
    with open(p, "wb") as fh:
        for f in frames:
            fh.write(struct.pack("<I", len(f)) + f)
    r = subprocess.run([exe, str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(frames)
    out = []
    for ln in lines:
        w, st, h = ln.split(" ", 3)[:3]
        out.append((int(w), int(st), int(h, 16)))
    return out


def test_shared_decoder_under_sanitizers(checker, tmp_path):
    L = _lib.lib()
    valid = zi.valid()
    frames = [f for _, _, f in valid]
    got = run_checker(checker, frames, tmp_path)
    for (label, data, _), (where, st, h) in zip(valid, got):
        assert (where, st) == (0, A.ZH_OK), label
        assert h == L.zh_xxh64(data, len(data), 0), label
    muts = zi.mutations()
    assert len(muts) == 1200
    got = run_checker(checker, muts, tmp_path)        # exit status 0: agreement on every frame
    shared = [g for g in got if g[0] == 0]
    assert len(shared) > 300                          # the shared decoder saw its part of them
    assert any(st == A.ZH_OK for _, st, _ in shared) and any(st != A.ZH_OK for _, st, _ in shared)
    corrupt = zi.corrupt()
    assert len(corrupt) >= 12
    got = run_checker(checker, [f for _, f in corrupt], tmp_path)
    for (label, f), (where, st, _) in zip(corrupt, got):
        assert st != A.ZH_OK, label
    # the corrupt frames reach the shared decoder, not only the header walk
    assert sum(1 for w, _, _ in got if w == 0) >= 12
    texts = {label: zi.host_decode(f)[2] for label, f in corrupt}
    assert texts["bad huffman weight sum"] == "zstd: Huffman weights do not complete a tree"
    assert texts["fse probabilities do not sum"] == \
        "zstd: FSE probabilities do not sum to the table size"
    assert texts["sequence code out of range"] == "zstd: RLE sequence code out of range"
    assert texts["offset before the frame"] == "zstd: match offset before the frame"
    assert texts["literals overrun"] == "zstd: sequence reads past the literals"
    assert texts["bitstream not consumed"] == "zstd: sequence bitstream not consumed exactly"
    assert texts["treeless without a table"] == \
        "zstd: treeless literals without a previous Huffman table"
    assert texts["repeat without a table"] == \
        "zstd: repeat sequence table without a previous table"
    assert texts["truncated jump table"] == "zstd: literals jump table truncated"
    assert texts["block larger than 128 KiB"] == "zstd: block larger than 128 KiB"
    assert texts["checksum mismatch"] == "zstd: content checksum mismatch"
