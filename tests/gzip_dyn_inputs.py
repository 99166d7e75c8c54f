"""Inputs and a reader for the gzip member writer with dynamic-Huffman segments
(test_gzip_dynamic_host.py on the host, test_gpu_gzip_dynamic.py on the device): the matrix of
gzip_enc_inputs.py with rows that the dynamic form is for, a walk over all three segment forms
that returns what a dynamic segment's header says, the writer's rules restated in Python (the
greedy run-length coding of the lengths, the sizes of the three forms from a histogram), a Python
Huffman for the cost of an optimal code, and the histograms of the code-length tests."""
import heapq
import struct

import numpy as np

import gzip_enc_inputs as gi
from gzip_enc_inputs import BLOCKSIZES, HEADER, LENGTH_BASES, MARKER, _DBASE, _LEXTRA

LITLEN, DIST = 286, 30
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_EXTRA = {16: 2, 17: 3, 18: 7}


def noisy(n=1 << 18):
    """The noisy image of test_gzip_encode_host.py: a random walk as <u2; the high bytes repeat,
    the low bytes are noise."""
    rng = np.random.default_rng(12)
    return np.cumsum(rng.integers(-40, 41, n // 2)).astype("<u2").tobytes()


def all_values():
    """300 bytes that hold all 256 byte values: a literal/length set with every literal."""
    return bytes(np.random.default_rng(24).permutation(256).astype(np.uint8)) + bytes(range(44))


def matrix():
    """gzip_enc_inputs.matrix() and, at each block size: the noisy image (64 KiB of it), one
    repeated 3-byte pattern (one distance code), a block shorter than 8 bytes (no match is
    looked for), 300 bytes of all 256 values."""
    rows = gi.matrix()
    for bs in BLOCKSIZES:
        rows.append((f"noisy-b{bs}", noisy(1 << 16), bs))
        rows.append((f"pattern3-b{bs}", b"abc" * 700, bs))
        rows.append((f"short-b{bs}", b"aabaaab", bs))
        rows.append((f"all_values-b{bs}", all_values(), bs))
    return rows


# (seed, bytes, alphabet, bits past 8 n - 10) of edge_rows(), found by a search over the seeds
EDGES = ((6538, 979, 205, 1), (7833, 671, 191, 2), (6709, 504, 169, 3), (5543, 335, 155, 4),
         (5231, 267, 130, 5), (5468, 128, 86, 6), (5134, 530, 174, 7), (9043, 35, 22, 1),
         (9139, 34, 24, 7))


def edge_rows():
    """Blocks whose dynamic segment is exactly n + 4 bytes, one under stored, with 8 n - 9 to
    8 n - 3 bits up to its end-of-block code: every place of that code in the segment's last
    byte before the marker.  (label, bytes, 1024, bits) rows of one block each."""
    rows = []
    for seed, n, alpha, past in EDGES:
        rng = np.random.default_rng(seed)       # the search drew the size, the alphabet, the bytes
        small = n < 64
        assert n == int(rng.integers(8, 48) if small else rng.integers(64, 1025))
        assert alpha == int(rng.integers(2, 40) if small else rng.integers(2, 257))
        data = rng.integers(0, alpha, n, dtype=np.uint8).tobytes()
        rows.append((f"edge-{n}-{past}", data, 1024, 8 * n - 10 + past))
    return rows


# ---- the rules, restated ------------------------------------------------------------------------
def len_extra(lc):
    return _LEXTRA[lc]


def dist_extra(dc):
    return max(0, dc // 2 - 1)


def sym_extra(s):
    """The extra bits behind symbol s of a 316-entry histogram (distance codes from 286)."""
    return 0 if s <= 256 else len_extra(s - 257) if s < LITLEN else dist_extra(s - LITLEN)


def fixed_len(s):
    return (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) if s < LITLEN else 5


def segment_bytes(bits):
    """Bytes of a fixed or dynamic segment whose bits up to the end-of-block code are `bits`."""
    return (bits + 3 + 7) // 8 + 4


def rle(lengths):
    """The greedy run-length coding of a header's lengths: [(symbol, extra value)]."""
    out, i = [], 0
    while i < len(lengths):
        v, run = lengths[i], 1
        while i + run < len(lengths) and lengths[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                t = min(run, 138)
                out.append((18, t - 11))
                run -= t
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                t = min(run, 6)
                out.append((16, t - 3))
                run -= t
        out += [(v, 0)] * run
    return out


def kraft(lens):
    """The Kraft sum of the non-zero lengths in units of 2^-15."""
    return sum(1 << (15 - n) for n in lens if n)


def huffman_cost(counts):
    """(cost in bits, depth) of an optimal prefix code over the used counts (two or more used).
    Ties go to the shallower subtree, so the depth is the least an optimal code needs."""
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


# ---- a reader of the writer's three segment forms -----------------------------------------------
def _decoder(lens):
    """(table, width): table[the next `width` stream bits] = symbol << 4 | length."""
    width = max(max(lens), 1)
    table = np.full(1 << width, -1, np.int32)
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, {}
    for n in range(1, 16):                                  # RFC 1951 §3.2.2
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    for sym, n in enumerate(lens):
        if n:
            c = nxt[n]
            nxt[n] += 1
            rev = int(format(c, f"0{n}b")[::-1], 2)
            table[rev::1 << n] = sym << 4 | n
    return table, width


class _Fast:
    """An LSB-first reader over a table decoder."""

    def __init__(self, data, bitpos):
        self.d, self.p = data, bitpos

    def peek(self, n):
        q = self.p >> 3
        return (int.from_bytes(self.d[q:q + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.p += n
        return v

    def sym(self, dec):
        e = int(dec[0][self.peek(dec[1])])
        assert e >= 0, "a code the set does not hold"
        self.p += e & 15
        return e >> 4


_FIXED = None


def _fixed_decoders():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _decoder([5] * 30))
    return _FIXED


def segments(member):
    """One dict per segment of a member the writer made.  All forms: "form" ("stored", "fixed"
    or "dynamic"), "raw" (bytes it decodes to) and "bytes" (its size).  Fixed and dynamic:
    "matches" [(length, distance, literals before it)], "hist" (316 counts: literal/length symbols,
    then distance codes; the end-of-block counted), "fixed_bytes" and "stored_bytes" (what the
    other forms would take).  Dynamic: "hlit", "hdist", "hclen" (the counts, not the fields),
    "cl_lens" (19), "cl_syms" [(symbol, extra value)] as sent, "ll_lens" and "d_lens" (untrimmed,
    286 and 30), "dyn_bytes" (recomputed from the header and the histogram).  Asserts the layout:
    the header, byte-aligned segments, the sync marker, the 03 00 ending, the trailer's place."""
    assert member[:10] == HEADER
    p, out = 10, []
    while member[p:p + 2] != b"\x03\x00" or p + 10 != len(member):
        start = p
        if member[p] == 0:                                  # stored, not final
            n, nn = struct.unpack("<HH", member[p + 1:p + 5])
            assert n ^ nn == 0xFFFF and n > 0
            p += 5 + n
            out.append({"form": "stored", "raw": n, "bytes": p - start})
            continue
        b = _Fast(member, 8 * p)
        assert b.take(1) == 0                               # BFINAL 0
        btype = b.take(2)
        assert btype in (1, 2)
        seg = {"form": "fixed" if btype == 1 else "dynamic"}
        if btype == 1:
            ll, dd = _fixed_decoders()
        else:
            hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
            assert hlit <= LITLEN and hdist <= DIST
            cl = [0] * 19
            for k in range(hclen):
                cl[CL_ORDER[k]] = b.take(3)
            cdec = _decoder(cl)
            syms, lens = [], []
            while len(lens) < hlit + hdist:
                s = b.sym(cdec)
                ex = b.take(CL_EXTRA.get(s, 0))
                syms.append((s, ex))
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + ex)
                else:
                    lens += [0] * ((3 if s == 17 else 11) + ex)
            assert len(lens) == hlit + hdist
            ll_lens = lens[:hlit] + [0] * (LITLEN - hlit)
            d_lens = lens[hlit:] + [0] * (DIST - hdist)
            header_bits = b.p - 8 * start - 3
            seg.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl, cl_syms=syms,
                       ll_lens=ll_lens, d_lens=d_lens)
            ll, dd = _decoder(ll_lens), _decoder(d_lens)
        hist = [0] * (LITLEN + DIST)
        nraw, nlit, matches = 0, 0, []
        while True:
            sym = b.sym(ll)
            hist[sym] += 1
            if sym == 256:
                break
            if sym < 256:
                nraw += 1
                nlit += 1
                continue
            assert sym <= 285
            ln = LENGTH_BASES[sym - 257] + b.take(_LEXTRA[sym - 257])
            dc = b.sym(dd)
            assert dc < 30
            hist[LITLEN + dc] += 1
            dist = _DBASE[dc] + b.take(dist_extra(dc))
            matches.append((ln, dist, nlit))
            nraw += ln
            nlit = 0
        seg["bits"] = b.p - 8 * start                       # up to and with the end of block
        assert b.take(3) == 0                               # the marker: BFINAL 0, BTYPE 00
        while b.p & 7:
            assert b.take(1) == 0
        p = b.p >> 3
        assert member[p:p + 4] == MARKER
        p += 4
        fixed_bits = 3 + sum(c * (fixed_len(s) + sym_extra(s)) for s, c in enumerate(hist))
        seg.update(raw=nraw, bytes=p - start, matches=matches, hist=hist,
                   fixed_bytes=segment_bytes(fixed_bits), stored_bytes=nraw + 5)
        if btype == 2:
            lens316 = ll_lens + d_lens
            seg["dyn_bytes"] = segment_bytes(3 + header_bits + sum(
                c * (lens316[s] + sym_extra(s)) for s, c in enumerate(hist)))
        out.append(seg)
    return out


# ---- histograms for the code-length tests -------------------------------------------------------
def fibonacci(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def histogram_sets():
    """[(label, nsym, limit, [rows of nsym counts])]: Fibonacci counts over 17..24 symbols (an
    optimal code is n - 1 deep: past 15 from 17 symbols on), the same over 19 symbols with limit
    7, one symbol, two symbols, 286 equal counts, and 200 seeded random histograms, some sparse."""
    rng = np.random.default_rng(77)
    sets = []
    for n in range(17, 25):
        rows = [fibonacci(n) + [0] * (LITLEN - n), [0] * (LITLEN - n) + fibonacci(n)[::-1]]
        sets.append((f"fibonacci-{n}", LITLEN, 15, rows))
    sets.append(("fibonacci-19-limit7", 19, 7, [fibonacci(19), fibonacci(19)[::-1]]))
    sets.append(("one", 30, 15, [[0] * 7 + [5] + [0] * 22, [0] * 29 + [1]]))
    sets.append(("two", 30, 15, [[3] + [0] * 28 + [900], [1, 1] + [0] * 28]))
    sets.append(("none", 30, 15, [[0] * 30]))
    sets.append(("equal", LITLEN, 15, [[7] * LITLEN]))
    rows = []
    for k in range(200):
        c = rng.integers(0, 1 << int(rng.integers(1, 22)), LITLEN)
        if k % 3 == 0:                                      # sparse
            c[rng.random(LITLEN) < 0.9] = 0
        if k % 7 == 0:                                      # a steep tail
            c = (c.astype(np.float64) ** 3 % (1 << 22)).astype(np.int64)
        rows.append([int(v) for v in c])
    sets.append(("random", LITLEN, 15, rows))
    sets.append(("random-19-limit7", 19, 7, [r[:19] for r in rows[:60]]))
    return sets
