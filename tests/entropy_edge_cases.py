"""Named inputs for the first-generation entropy coders (ANS0, ANS1, HUFFMAN, FPAQ) at the edges their kernels hard-code: chunks of
16 KiB (ANS1: 4 MiB) and 16 chunk slots per decode wave, 4 lanes / fragments / quarters per chunk, the raw path up to 32 bytes and
Huffman's raw tail chunk below 32, frequency groups of 6 symbols below 64 symbols and of 8 from 64 up, presence masks / the no-mask
form at 256 symbols / the fill path at 1 symbol, n == 4096 (order 0) and a context total of 2048 (order 1) skipping normalisation,
the 1 KiB header window with its guessed prefetch, the 56-bit window for Huffman's length deltas, its 10-bit primary and 512-entry
overflow table, FPAQ's publication every 64 KiB and its sub-chunks of 4 MiB.

A stage case is (name, bytes, property); `property` says what the case is there for and tests/test_entropy_edges.py derives it
again from the bytes. Everything is drawn from fixed seeds; nothing is read from the file system. The reference's output for
every case is pinned in tests/golden/entropy_edges.json (tests/golden/make_entropy_edges.py)."""
import functools
import zlib

import numpy as np

import knzlib

CH = 16384
M4 = 4 << 20
CODERS = ("ANS0", "ANS1", "HUFFMAN", "FPAQ")
EMU_MAX = 2 * CH + 1          # the emulator harnesses take the stage cases up to this size

LENGTHS = (32, 33, 34, 35, 36, 37, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, CH - 1, CH, CH + 1, CH + 2, CH + 3, CH + 4,
           CH + 31, CH + 32, CH + 33, CH + 4096, 2 * CH - 1, 2 * CH, 2 * CH + 1, 15 * CH, 16 * CH - 1, 16 * CH, 16 * CH + 1, 17 * CH + 5,
           64 * CH, 64 * CH + 1, 65535, 65536, 65537)
ALPHABET_SIZES = (1, 2, 3, 6, 7, 8, 9, 62, 63, 64, 65, 66, 127, 128, 129, 254, 255, 256)
PLACEMENTS = ("low", "high", "random")
M4_CUTS = (M4 - 1, M4, M4 + 1, M4 + 2, M4 + 3, M4 + 4, M4 + 7, M4 + 33)
FPAQ_M4_CUTS = (M4 - 1, M4, M4 + 1)

BATCH_BLOCKS = 18
BATCH_BLOCK_SIZES = (CH + 16, 2 * CH, 3 * CH, 5 * CH)
BATCH_TAILS = (0, 1, 15, 16, 32, 33, CH + 5)
BATCH_CHECKSUMS = (0, 32)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _weights(k, skewed):
    """Probabilities over k ranks: uniform, or geometric with a floor (rank 0 about a tenth of the mass at 200 ranks)."""
    if not skewed:
        return np.full(k, 1.0 / k)
    w = 0.97 ** np.arange(k) + 0.01
    return w / w.sum()


def draw(rng, symbols, n, skewed, cover):
    """n bytes over `symbols` (their order is the rank order of a skewed draw); with `cover` every symbol occurs at least once."""
    symbols = np.asarray(symbols, dtype=np.uint8)
    k = len(symbols)
    if cover:
        assert n >= k
        out = np.concatenate([symbols, symbols[rng.choice(k, size=n - k, p=_weights(k, skewed))]])
        rng.shuffle(out)
    else:
        out = symbols[rng.choice(k, size=n, p=_weights(k, skewed))]
    return out.tobytes()


def alphabet(rng, k, place):
    """k byte values at the bottom of the range, at its top, or anywhere, in a drawn rank order."""
    if place == "low":
        s = np.arange(k)
    elif place == "high":
        s = np.arange(256 - k, 256)
    else:
        s = rng.choice(256, size=k, replace=False)
    return rng.permutation(s).astype(np.uint8)


def pow2_chunk(rng, nsym):
    """Frequencies 1, 2, 4, ... 2^(nsym-1) on drawn symbols: no two equal and no merged weight equal to a frequency, so the optimal
    code is unique in its lengths, 1, 2, ... nsym-1, nsym-1."""
    sym = rng.choice(256, size=nsym, replace=False)
    out = np.concatenate([np.full(1 << i, sym[i], dtype=np.uint8) for i in range(nsym)])
    rng.shuffle(out)
    return out.tobytes()


def _length_cases():
    rng = _rng("lengths")
    sym = alphabet(rng, 200, "random")
    return [("len:%d" % n, draw(rng, sym, n, True, False), {"len": n, "last_chunk": (n - 1) % CH + 1, "chunks": (n + CH - 1) // CH})
            for n in LENGTHS]


def _alphabet_cases():
    out = []
    for k in ALPHABET_SIZES:
        for place in PLACEMENTS if k < 256 else PLACEMENTS[:1]:          # (at 256 symbols the placements are one)
            for kind, n in (("two", CH + 777), ("short", max(k, 33) + 5)):
                name = "asz:%d:%s:%s" % (k, place, kind)
                rng = _rng(name)
                sym = alphabet(rng, k, place)
                d = b"".join(draw(rng, sym, min(CH, n - at), k > 8, True) for at in range(0, n, CH))
                out.append((name, d, {"asz": k, "place": place, "len": n}))
    return out


def _kinds_block():
    rng = _rng("kinds")
    parts = [bytes([0x41]) * CH, rng.integers(0, 256, CH, dtype=np.uint8).tobytes(), bytes([0x7A]) * CH,
             draw(rng, [3, 150, 251], CH, False, True), draw(rng, alphabet(rng, 255, "random"), CH, True, True), bytes([0xEE]) * 100]
    return [("kinds", b"".join(parts), {"chunk_asz": [1, 256, 1, 3, 255, 1]})]


def _huffman_cases():
    out = []
    rng = _rng("huffman")
    lead = draw(rng, alphabet(rng, 200, "random"), CH, True, False)
    # 14 symbols at 1, 2, ... 8192: the optimal code is 13 bits deep, the length limiter cuts it to 12; second chunk of its block
    out.append(("huff:limit", lead + pow2_chunk(rng, 14), {"chunk": 1, "optimal_len": 13, "max_code_len": 12}))
    for depth in (10, 11, 12):
        out.append(("huff:max%d" % depth, pow2_chunk(rng, depth + 1), {"chunk": 0, "optimal_len": depth, "max_code_len": depth}))
    # 1/2, 1/4, 1/8 and 253 equally rare symbols: codes of 11 and 12 bits all over the overflow table
    sym = rng.permutation(256).astype(np.uint8)
    counts = [8192, 4096, 2048] + [9] * 24 + [8] * 229
    d = np.concatenate([np.full(c, s, dtype=np.uint8) for s, c in zip(sym, counts)])
    rng.shuffle(d)
    out.append(("huff:dominant3", d.tobytes(), {"chunk": 0, "asz": 256, "long_codes": 240}))
    # 140 codes of 10 bits in front of 24 of 11 (one symbol at 1/2, 90 at 1/256, 140 at 1/1024, 24 at 1/2048: powers of two, so the
    # lengths are theirs whatever the ties): the 12-bit slots from the first 10-bit code on are more than the overflow table has, and
    # the next chunk's table is full of long codes
    sym = rng.permutation(256).astype(np.uint8)
    counts = [8192] + [64] * 90 + [16] * 140 + [8] * 24
    d0 = np.concatenate([np.full(c, s, dtype=np.uint8) for s, c in zip(sym, counts)])
    rng.shuffle(d0)
    d1 = np.frombuffer(d.tobytes(), dtype=np.uint8).copy()
    rng.shuffle(d1)
    out.append(("huff:ten_then_long", d0.tobytes() + d1.tobytes(), {"chunk": 0, "asz": 255, "slots_from_10": 608, "next_long_slots": 448}))
    # even symbols 120 times, odd ones 8 times: the lengths go up and down by four from symbol to symbol
    d = np.concatenate([np.full(120 if s % 2 == 0 else 8, s, dtype=np.uint8) for s in range(256)])
    rng.shuffle(d)
    out.append(("huff:alternate", d.tobytes(), {"chunk": 0, "asz": 256, "delta_bits": 4 * 56}))
    return out


def _ans1_cases():
    out = []
    # context bytes A, B, C followed (inside a quarter) 2048, 2047 and 2049 times by a skewed symbol: pairs that never straddle a quarter
    rng = _rng("ans1:ctx2048")
    A, B, C = 0x10, 0x80, 0xF0
    follow = np.array([0x21 + 3 * i for i in range(20)], dtype=np.uint8)
    filler = np.array([0x05, 0x06, 0x07], dtype=np.uint8)
    quarters = []
    for q, (na, nb, nc) in enumerate(((512, 512, 513), (512, 512, 512), (512, 512, 512), (512, 511, 512))):
        heads = np.concatenate([np.full(na, A), np.full(nb, B), np.full(nc, C)]).astype(np.uint8)
        heads = np.concatenate([heads, filler[rng.integers(0, 3, 2048 - len(heads))]])
        rng.shuffle(heads)
        w = 0.8 ** np.arange(20)
        tails = follow[rng.choice(20, size=2048, p=w / w.sum())]
        quarters.append(np.stack([heads, tails], axis=1).reshape(-1))
    out.append(("ans1:ctx2048", np.concatenate(quarters).tobytes(), {"ctx_totals": {A: 2048, B: 2047, C: 2049}}))
    rng = _rng("ans1:sparse")
    out.append(("ans1:sparse", draw(rng, [3, 77, 200, 255], CH + 777, True, True), {"contexts": 5}))
    mixed = knzlib.corpus().mixed(M4 + 33, 7)
    for n in M4_CUTS:
        out.append(("m4:%d" % n, mixed[:n], {"len": n, "last_chunk_ans1": (n - 1) % M4 + 1}))
    return out


@functools.lru_cache(maxsize=None)
def stage_cases():
    """Every stage case, in the fixture's order: [(name, bytes, property)]."""
    cases = _length_cases() + _alphabet_cases() + _kinds_block() + _huffman_cases() + _ans1_cases()
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def device_coders(name, data):
    """The coders a stage case goes to on the device: the 4 MiB cuts belong to ANS1 (all of them) and FPAQ (three); ANS0 and HUFFMAN
    get nothing above 64 * CH + 1 bytes."""
    if len(data) <= 64 * CH + 1:
        return CODERS
    return ("ANS1", "FPAQ") if len(data) in FPAQ_M4_CUTS else ("ANS1",)


def offset_case(name, prop):
    """The cases whose decode is repeated at odd bit offsets: header windows and fill paths depend on the alignment."""
    return prop.get("asz") in (1, 63, 64, 65, 256) and name.startswith("asz:") or name in ("len:33", "len:%d" % (CH + 1), "len:%d" % (CH + 33))


@functools.lru_cache(maxsize=None)
def batch_master():
    """16 KiB pieces that cycle constant, noise, text, three symbols, geometric."""
    rng = _rng("batch")
    c = knzlib.corpus()
    text = c.text(40 * CH, 11)
    pieces = []
    for i in range(BATCH_BLOCKS * 5 + 2):
        kind = i % 5
        if kind == 0:
            pieces.append(bytes([(37 * i + 5) & 255]) * CH)
        elif kind == 1:
            pieces.append(rng.integers(0, 256, CH, dtype=np.uint8).tobytes())
        elif kind == 2:
            pieces.append(text[(i // 5) * CH:(i // 5 + 1) * CH])
        elif kind == 3:
            pieces.append(draw(rng, [9, 10, 200], CH, False, True))
        else:
            pieces.append(bytes((rng.geometric(0.08, CH) % 256).astype(np.uint8)))
    return b"".join(pieces)


def batch_inputs():
    """[(name, block size, bytes)]: 18 blocks and a tail."""
    m = batch_master()
    return [("batch:%d+%d" % (bs, tail), bs, m[:BATCH_BLOCKS * bs + tail]) for bs in BATCH_BLOCK_SIZES for tail in BATCH_TAILS]


def batch_key(name, coder, checksum):
    return "%s:%s:x%d" % (name, coder, checksum)


# ---- what the tests derive from the bytes

def chunk_alphabets(data, chunk=CH):
    return [len(set(data[at:at + chunk])) for at in range(0, len(data), chunk)]


def order1_context_totals(chunk):
    """Symbols counted per context by the order-1 histogram of one ANS1 chunk: four quarters of len >> 2 bytes, the first byte of a
    quarter in context 0, the len & 3 tail bytes not at all; a chunk of fewer than 4 bytes is one quarter."""
    a = np.frombuffer(chunk, dtype=np.uint8)
    q = len(a) >> 2
    parts = [a[i * q:(i + 1) * q] for i in range(4)] if q else [a]
    tot = np.zeros(256, dtype=np.int64)
    for p in parts:
        if len(p):
            tot[0] += 1
            tot += np.bincount(p[:-1], minlength=256)
    return tot


def huffman_lengths(freqs):
    """Plain Huffman code lengths of a {symbol: count} table, and whether any choice between equal weights was met on the way."""
    import heapq
    heap = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freqs.items()))]
    heapq.heapify(heap)
    lens = dict.fromkeys(freqs, 0)
    tie, n = False, len(heap)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        tie |= a[0] == b[0] or (bool(heap) and heap[0][0] == b[0])
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], n, a[2] + b[2]))
        n += 1
    return lens, tie


class _Bits:
    def __init__(self, data):
        self.v, self.n, self.pos = int.from_bytes(data, "big"), 8 * len(data), 0

    def get(self, k):
        assert self.pos + k <= self.n
        self.pos += k
        return (self.v >> (self.n - self.pos)) & ((1 << k) - 1) if k else 0

    def varint(self):
        res, shift = 0, 0
        while True:
            b = self.get(8)
            res |= (b & 0x7F) << shift
            shift += 7
            if b < 128:
                return res


def huffman_chunk_headers(enc, n):
    """Walks a HUFFMAN stream of n bytes (current bitstream version): per 16 KiB chunk None for a raw chunk, or ({symbol: code
    length}, bits of the length deltas)."""
    r, out = _Bits(enc), []
    for at in range(0, n, CH):
        size = min(CH, n - at)
        if size < 32:
            r.get(8 * size)
            out.append(None)
            continue
        if r.get(1) == 0:
            syms = list(range(256)) if r.get(1) == 0 else []
        else:
            last = r.get(5)
            masks = [r.get(8) for _ in range(last + 1)]
            syms = [8 * i + j for i in range(last + 1) for j in range(8) if (masks[i] >> j) & 1]
        start, cur, lens = r.pos, 2, {}
        for s in syms:
            if r.get(1) == 0:
                lg = 1
                while r.get(1) == 0:
                    lg += 1
                v = r.get(lg + 1)
                sgn = v & 1
                v = (v >> 1) + (1 << lg) - 1
                cur += -v if sgn else v
            lens[s] = cur
        out.append((lens, r.pos - start))
        if len(syms) > 1:
            frag = [r.varint() for _ in range(4)]
            r.get(sum(frag))
            r.get(8 * (size & 3))
    return out
