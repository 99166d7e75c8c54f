"""zh_zstd_decompress against recorded verdicts (tests/golden/zstd_verdicts.txt): the size query's
status and byte count, the decode's status, the hash of the decoded bytes and the message of
every frame of own_corpus().  No GPU, and no libzstd makes any of the frames."""
import ctypes as C
import functools
import os
import struct

import numpy as np

import zstd_dec_inputs as zi
from helpers import GOLDEN
from zarrhip import _abi as A
from zarrhip import _lib

VERDICTS = os.path.join(GOLDEN, "zstd_verdicts.txt")
# A mutated header may declare any content size; the decode gets a destination of at most this.
MAX_DST = 4 << 20


OWN_MUTATIONS = 800


def own_valid():
    """The entries of zi.valid() that no installed libzstd has a hand in: the library's own
    frames, the OME fixtures and the hand-built frames."""
    return [v for v in zi.valid() if not v[0].startswith("libzstd")]


def own_host_routed():
    """[(label, frame)]: zi.host_routed() rebuilt from the library's own frames."""
    ds = zi.datasets()
    a = _lib.zstd_compress(ds["text"], True, 1 << 10)
    b = _lib.zstd_compress(ds["walk"][:5000], False, 16 << 10)
    skip = b"\x50\x2a\x4d\x18" + struct.pack("<I", 5) + b"hello"
    nofcs = zi.MAGIC + b"\x00\x58" + zi.hand_blocks()[1][9:]     # as zi.host_routed() makes it
    return [("own concatenated", a + b), ("own skippable then frame", skip + a),
            ("own frame then skippable", a + skip), ("no content size", nofcs)]


def own_mutations(n=OWN_MUTATIONS, seed=78):
    """zi.mutations() over own_valid(): the same three kinds in the same draw order."""
    rng = np.random.default_rng(seed)
    pool = [f for _, _, f in own_valid() if 0 < len(f) <= 40000]
    out = []
    for k in range(n):
        f = bytearray(pool[int(rng.integers(0, len(pool)))])
        kind = k % 3
        pos = int(rng.integers(0, len(f)))
        if kind == 0:
            f[pos] = int(rng.integers(0, 256))
        elif kind == 1:
            f = f[:pos]
        else:
            f[pos] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(f))
    return out


@functools.lru_cache(maxsize=None)
def own_corpus():
    """[(label, frame)]: the frames whose verdicts the golden file records.  No frame depends on
    the libzstd installed here: own_valid(), own_host_routed(), zi.corrupt() without the flipped
    libzstd frame, zi.impossible_size(), and the mutations (the last OWN_MUTATIONS entries)."""
    out = [(label, f) for label, _, f in own_valid()] + own_host_routed()
    out += [c for c in zi.corrupt() if c[0] != "flipped bit mid-frame"]
    out.append(("impossible size", zi.impossible_size()))
    return out + [(f"mutation {k}", f) for k, f in enumerate(own_mutations())]


def xxh(b):
    return _lib.lib().zh_xxh64(bytes(b), len(b), 0)


def verdict(frame):
    """The golden line of one frame, without the frame's hash."""
    st, nb, msg = zi.size_query(frame)
    if st != A.ZH_OK:
        return f"{st} - - {0:016x} {msg}"      # the byte count of a failed call says nothing
    cap = min(nb, MAX_DST)
    out = C.create_string_buffer(max(1, cap))
    n = C.c_size_t()
    err = C.create_string_buffer(256)
    ds = _lib.lib().zh_zstd_decompress(bytes(frame), len(frame), out, cap, C.byref(n), err, 256)
    h = xxh(out.raw[:n.value]) if ds == A.ZH_OK else 0
    return f"{st} {nb} {ds} {h:016x} {err.value.decode()}"


def record():
    """Writes tests/golden/zstd_verdicts.txt from the library that is built now.  The committed
    file was recorded from the parent of the commit that made zh_zstd_dec.h the only decoder,
    that is from the former host decoder of zh_zstd.cpp; it is not recorded again from a later
    library unless a change of verdicts is the purpose of that commit.  No test calls it; in tests/:
    python -c "import conftest, test_zstd_golden; test_zstd_golden.record()" """
    lines = {}
    for _, f in own_corpus():
        lines.setdefault(f"{xxh(f):016x}", verdict(f))
    with open(VERDICTS, "w") as fh:
        fh.write("# xxh64(frame) size-query-status size decode-status xxh64(decoded) message\n")
        fh.writelines(f"{h} {v}".rstrip() + "\n" for h, v in lines.items())
    print(len(lines), "lines")


def golden():
    with open(VERDICTS) as fh:
        return dict(ln.rstrip("\n").split(" ", 1) for ln in fh if not ln.startswith("#"))


def test_verdicts_equal_the_recorded_ones():
    want = golden()
    corpus = own_corpus()
    assert len(corpus) == 31 + 4 + 15 + 1 + OWN_MUTATIONS
    for label, f in corpus:
        h = f"{xxh(f):016x}"
        assert h in want, f"{label}: no recorded verdict for this frame: the encoder's output " \
            "(or a fixture, or the construction of the corpus) changed"
        assert verdict(f).rstrip() == want[h], label


def test_mutations_reach_the_decoder():
    """Conditions on the corpus, not measurements: the mutations are rejected for many reasons,
    many still decode, and many are frames the plan sends to the device."""
    muts = [f for _, f in own_corpus()[-OWN_MUTATIONS:]]
    assert len(muts) == 800
    texts, accepted, device = set(), 0, 0
    for f in muts:
        st, nb, ds, _, msg = (verdict(f).split(" ", 4) + [""])[:5]
        if (st, ds) == ("0", "0"):
            accepted += 1
        else:
            texts.add(msg)
        if st == "0":
            device += _lib.zstd_batch_plan([f])[1][0][2] == 0
    assert len(texts) >= 20 and accepted >= 150 and device >= 300, (len(texts), accepted, device)
