"""Inputs of the ROLZX tests, rebuilt from short recipes: tests/golden/rolzx.json stores the recipes and what the pinned model
(tests/rolzx_model.py) or the reference computed from them (tools/make_rolzx_golden.py), the tests rebuild the bytes. A recipe is
[kind, size, seed, ...]."""
import numpy as np

CHUNK = 1 << 24


def max_encoded(n):
    """ROLZCodec2::getMaxEncodedLength"""
    return n + (1024 if n < 32768 else n >> 5)


def _len(ops):
    return sum(o[2] if o[0] in ("a", "z") else (len(o[1]) // 2 if o[0] == "x" else o[1]) for o in ops)


def _seq(n, seed, ops):
    """Bytes laid down piece by piece: ["r", len] random bytes below 240, ["R", len] random bytes, ["a", offset, len] a copy from that
    offset (byte by byte, so it may overlap itself), ["x", hex], ["z", byte, len]."""
    rng = np.random.default_rng(seed)
    d = bytearray()
    for op in ops:
        if op[0] == "r":
            d += rng.integers(0, 240, op[1], dtype=np.uint8).tobytes()
        elif op[0] == "R":
            d += rng.integers(0, 256, op[1], dtype=np.uint8).tobytes()
        elif op[0] == "a":
            for i in range(op[2]):
                d.append(d[op[1] + i])
        elif op[0] == "x":
            d += bytes.fromhex(op[1])
        elif op[0] == "z":
            d += bytes([op[1]]) * op[2]
        else:
            raise ValueError(op)
    assert len(d) == n, (len(d), n, ops)
    return bytes(d)


def text(n, seed):
    """Words drawn from a pool of 200 with spaces and line ends: many short and medium repeats."""
    rng = np.random.default_rng(seed)
    pool = [rng.integers(97, 123, int(rng.integers(2, 10)), dtype=np.uint8).tobytes() for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += pool[int(rng.integers(0, 200)) if rng.random() < 0.8 else int(rng.integers(0, 12))]
        out += b"\n" if rng.random() < 0.1 else b" "
    return bytes(out[:n])


def make(recipe):
    kind, n, seed = recipe[0], recipe[1], recipe[2]
    if kind == "seq":
        return _seq(n, seed, recipe[3])
    if kind == "rnd":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "const":
        return bytes([seed & 255]) * n
    if kind == "period":
        unit = np.random.default_rng(seed).integers(0, 240, recipe[3], dtype=np.uint8).tobytes()
        return (unit * (n // recipe[3] + 1))[:n]
    if kind == "text":
        return text(n, seed)
    if kind == "phrase":
        # a short text repeated to the size: the chunk test's input (highly compressible: matches of the maximum throughout)
        unit = text(recipe[3], seed)
        return (unit * (n // len(unit) + 1))[:n]
    if kind == "sym":
        syms = np.frombuffer(bytes.fromhex(recipe[3]), dtype=np.uint8)
        return syms[np.random.default_rng(seed).integers(0, len(syms), n)].tobytes()
    if kind == "dna":
        # random ACGT with repeats of earlier stretches: DNA for detectSimpleType, matches of 7 and more through getKey2
        rng = np.random.default_rng(seed)
        syms = np.frombuffer(b"ACGT", dtype=np.uint8)
        d = bytearray(syms[rng.integers(0, 4, 300)].tobytes())
        while len(d) < n:
            if rng.random() < 0.5:
                o, k = int(rng.integers(0, len(d) - 8)), int(rng.integers(6, 120))
                for i in range(k):
                    d.append(d[o + i])
            else:
                d += syms[rng.integers(0, 4, int(rng.integers(5, 60)))].tobytes()
        return bytes(d[:n])
    if kind == "elf":
        # the ELF magic in front of text with a few opcode-like bytes: EXE by the block's magic in a stream
        body = bytearray(text(n - 4, seed))
        for p in range(50, len(body) - 5, 97):
            body[p:p + 5] = bytes([0xE8, p & 255, (p >> 8) & 255, 0, 0])
        return b"\x7fELF" + bytes(body)
    if kind == "fill":
        # another recipe's bytes, then text up to the size
        head = make(recipe[3])
        return head + text(n - len(head), seed)
    if kind == "concat":
        return b"".join(make(r) for r in recipe[3])
    raise ValueError(kind)


def _hash0_triple():
    """Three bytes whose hash32 is 0 (the low three bytes decide; found by search)."""
    w = np.arange(1 << 24, dtype=np.uint64)
    h = (((w << np.uint64(8)) & np.uint64(0xFFFFFFFF)) * np.uint64(200002979)) & np.uint64(0xFF000000)
    for v in np.flatnonzero(h == 0):
        b = int(v).to_bytes(3, "little")
        if all(0 < x < 240 for x in b) and len(set(b)) == 3:
            return b
    raise AssertionError


PAD = 800


def _padded(ops, seed):
    """The pieces behind a run of 800 spaces (which makes the block compressible enough to be accepted); copies count from the run's end."""
    ops = [["z", 0x20, PAD]] + [["a", o[1] + PAD, o[2]] if o[0] == "a" else o for o in ops]
    return ["seq", _len(ops), seed, ops]


def _match(length, pre=200, post=60):
    """`pre` random bytes, then a repeat of two context bytes and `length` bytes of them, then `post` random bytes."""
    return _padded([["r", pre], ["r", 16], ["a", 40, 2 + length]] + ([["r", post]] if post else []), 3000 + length)


def _overshoot_behind_exact():
    """Three passages with one two-byte context. The first has 300 bytes S, the second S's first 250 and then another byte, the third S
    again far from the block's end (maxMatch 250): the newest candidate reaches 250 exactly and ends the scan; the older one, whose
    word-stepped length is 256, does not get to win."""
    return _padded([["r", 100], ["x", "f1f2"], ["r", 300], ["r", 50], ["x", "f1f2"], ["a", 102, 250], ["x", "ff"], ["r", 20], ["r", 50],
                    ["x", "f1f2"], ["a", 102, 300], ["r", 400]], 3100)


def _equal_lengths():
    """Two earlier passages that agree with the third in 20 bytes each: the newer one (index 0) wins."""
    return _padded([["r", 100], ["x", "f3f4"], ["r", 20], ["x", "f5"], ["r", 40], ["x", "f3f4"], ["a", 102, 20], ["x", "f6"], ["r", 40],
                    ["x", "f3f4"], ["a", 102, 20], ["x", "f7"], ["r", 100]], 3200)


def _zero_entry():
    """The block starts with three bytes whose hash32 is 0 and ten more; the same 13 bytes return behind a context that no position has
    had: every entry of that ring is still zero, which reads as position 0 with hash 0, so the passage is a match with position 0."""
    t = _hash0_triple().hex()
    ops = [["x", t], ["r", 10], ["z", 0x20, PAD], ["r", 120], ["x", "f8f9"], ["a", 0, 13], ["r", 80]]
    return ["seq", _len(ops), 3300, ops]


def damage(fwd, op):
    """A forward output as a damaged record has it: ["whole"], ["cut", length], ["flip", position, xor], ["len", added to the length field]"""
    if op[0] == "whole":
        return fwd
    if op[0] == "cut":
        return fwd[:op[1]]
    if op[0] == "flip":
        return fwd[:op[1]] + bytes([fwd[op[1]] ^ op[2]]) + fwd[op[1] + 1:]
    if op[0] == "len":
        return (int.from_bytes(fwd[:4], "big") + op[1]).to_bytes(4, "big") + fwd[4:]
    raise ValueError(op)


STAGE = (
    [["const", n, 0x41] for n in (0, 63, 64, 65, 72)]
    + [["period", n, 7, 5] for n in (64, 65, 72, 200)]
    + [["text", 72, 9], ["text", 1000, 10], ["text", 4097, 11], ["text", 20000, 12], ["period", 3000, 13, 1], ["period", 5000, 14, 300]]
    + [_match(2), _match(3), _match(4), _match(249), _match(250), _match(251), _match(600), _match(40, 200, 0), _match(40, 200, 7)]
    + [_overshoot_behind_exact(), _equal_lengths(), _zero_entry()]
    + [["rnd", 64, 40], ["rnd", 4096, 41], ["sym", 3000, 42, "4142"], ["sym", 300, 43, "30313233343536373839"],
       ["dna", 64, 50], ["dna", 3000, 51], ["dna", 10000, 52], ["elf", 3000, 60]]
)
# stage records with a preset data type: [recipe, data type] (3 EXE, 6 DNA, 1 TEXT)
PRESET = [[["text", 4097, 11], 3], [["text", 4097, 11], 6], [["text", 4097, 11], 1], [["dna", 3000, 51], 6], [["dna", 3000, 51], 3], [["elf", 3000, 60], 3]]
SHORT_CAP = ["text", 4097, 11]            # also run with a destination one byte below the bound (refused, ROLZCodec.cpp:916)

# forward outputs of these are cut and damaged for the inverse
CUT_FROM = [["text", 4097, 11], ["dna", 3000, 51], _match(600), ["period", 200, 7, 5]]

CHUNK_PHRASE = 173
CHUNKS = [["phrase", CHUNK + extra, 70, CHUNK_PHRASE] for extra in (0, 1, 12, 100000)]

STREAM_BS = 65536
STREAM = ["concat", 7 * 65536 + 10, 0, [["text", 65536, 80], ["rnd", 65536, 81], ["dna", 65536, 82], ["elf", 65536, 83],
                                         ["text", 65536, 84], ["period", 65536, 85, 700], ["sym", 65536, 86, "41434754"], ["rnd", 10, 87]]]
STREAM_CHAINS = [("ROLZX", "NONE", 0), ("ROLZX", "HUFFMAN", 0), ("PACK+ROLZX", "ANS0", 0), ("ROLZX+RLT", "FPAQ", 0), ("ROLZX", "ANS0", 32)]
# a batch of 71 blocks of 4,096 bytes (the last one 100) in which no two neighbours are alike: every kind of stage record, filled up with text
RAGGED_BS = 4096
_KINDS = ([["fill", 4096, 100 + i, r] for i, r in enumerate(STAGE) if 64 <= r[1] <= 4096 and r[0] != "rnd"]
          + [["rnd", 4096, 41], ["dna", 4096, 53], ["elf", 4096, 61], ["text", 4096, 15], ["period", 4096, 16, 9], ["const", 4096, 0x41]])
RAGGED = ["concat", 70 * 4096 + 100, 0, [_KINDS[i % len(_KINDS)] for i in range(70)] + [["text", 100, 17]]]
HOSTED = [("TEXT+ROLZX", "HUFFMAN", 65536, 0, ["concat", 3 * 65536 + 500, 0, [["text", 3 * 65536 + 500, 90]]])]
CLI = ["concat", 300007, 0, [["text", 200000, 91], ["rnd", 30000, 92], ["period", 70007, 93, 500]]]
