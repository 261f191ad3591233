"""Inputs of the LZP tests, rebuilt from short recipes: tests/golden/lzp.json stores the recipes and what the reference computed from
them (tools/make_lzp_golden.py), the tests rebuild the bytes. A recipe is [kind, size, seed, ...]."""
import numpy as np


def max_encoded(n):
    """LZPCodec::getMaxEncodedLength"""
    return n + 16 if n <= 1024 else n + n // 64


def _seq(n, seed, ops):
    """Bytes laid down piece by piece: ["r", len] random bytes below 240, ["R", len] random bytes, ["F", len, percent] 0xFC with that
    probability and 'A' otherwise, ["a", offset, len] a copy from that offset (byte by byte, so it may overlap itself), ["x", hex],
    ["z", byte, len]."""
    rng = np.random.default_rng(seed)
    d = bytearray()
    for op in ops:
        if op[0] == "r":
            d += rng.integers(0, 240, op[1], dtype=np.uint8).tobytes()
        elif op[0] == "R":
            d += rng.integers(0, 256, op[1], dtype=np.uint8).tobytes()
        elif op[0] == "F":
            d += np.where(rng.random(op[1]) * 100 < op[2], 0xFC, 0x41).astype(np.uint8).tobytes()
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
    """Paragraphs of lower-case letters drawn from a pool of 12: long repeats at predictable places."""
    rng = np.random.default_rng(seed)
    pool = [rng.integers(97, 123, int(rng.integers(90, 400)), dtype=np.uint8).tobytes() + b"\n" for _ in range(12)]
    out = bytearray()
    while len(out) < n:
        out += pool[int(rng.integers(0, 12))]
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
    if kind == "sym":
        # random bytes over a few symbols (hex string): contexts repeat at once, so buckets are filled and 64-byte repeats never happen
        syms = np.frombuffer(bytes.fromhex(recipe[3]), dtype=np.uint8)
        return syms[np.random.default_rng(seed).integers(0, len(syms), n)].tobytes()
    if kind == "concat":
        return b"".join(make(r) for r in recipe[3])
    raise ValueError(kind)


def _match(length, tail=100, pre=None):
    """400 random bytes (and the pieces of `pre`), then 4 bytes that bring the context in step and a repeat of `length` bytes of them, then
    `tail` random bytes."""
    ops = [["r", 400 if length < 300 else length + 400]] + (pre or []) + [["r", 16], ["a", 96, 4 + length]] + ([["r", tail]] if tail else [])
    return ["seq", _len(ops), 1000 + length, ops]


def _mixed_after_match(k):
    """A repeat found k literals behind a match. Every passage is the same match (a copy of 4 + 104 bytes) and what follows it. The first
    (k literals of 0xF0.., 80 bytes D) stores D's position under the mixed context. Spoilers (the first j < k literals, then other bytes)
    take over the buckets of the visits in front of D; a passage with no literal in common stands in front of every other one, so that
    each match ends where the copy ends. The last passage finds D only at the k-th literal."""
    lits = "f0f1f2"[:2 * k]
    copy = [["r", 16], ["a", 92, 108]]
    ops = [["r", 300]] + copy + [["x", lits]]
    d_at = _len(ops)
    ops += [["r", 80]]
    for j in range(1, k):
        ops += copy + [["r", 80]] + copy + [["x", lits[:2 * j]], ["r", 80]]
    ops += copy + [["r", 80]] + copy + [["x", lits], ["a", d_at, 80], ["r", 120]]
    return ["seq", _len(ops), 2000 + k, ops]


def _len(ops):
    return sum(o[2] if o[0] in ("a", "z") else (len(o[1]) // 2 if o[0] == "x" else o[1]) for o in ops)


def _mixed_after_start():
    """Three repeats whose bucket was stored 1, 2 and 3 literals behind the block start: the four bytes in front of each repeat spell the
    mixed context of position 5, 6 and 7 in the order a plain context reads them."""
    ops = [["r", 400]]
    for k, ctx in ((1, (2, 1, 0, 4)), (2, (1, 0, 4, 5)), (3, (0, 4, 5, 6))):
        ops += [["r", 16]] + [["a", o, 1] for o in ctx] + [["a", 4 + k, 70], ["r", 30]]
    return ["seq", _len(ops), 2100, ops]


def _back_to_back():
    """A match that ends in four equal bytes (the reloaded context reads the same in both byte orders) with a second repeat right behind it."""
    ops = [["r", 100], ["x", "eeeeeeee"], ["r", 80], ["r", 20], ["x", "eeeeeeee"]]
    y_at = _len(ops)
    ops += [["r", 80], ["r", 16], ["a", 0, 104], ["a", y_at, 80], ["r", 150]]
    return ["seq", _len(ops), 2200, ops]


def _fe_run_refused(fl):
    """Random bytes, a stretch rich in escaped 0xFC that brings the output up to the limit, then a long repeat whose 0xFE run crosses it."""
    ops = [["R", 10400], ["F", fl, 50], ["r", 8], ["a", 92, 8 + 10224]]
    return ["seq", _len(ops), 2300, ops]


FE_RUN_FL = 19250          # chosen with tests/lzp_model.py: the output stands within 40 bytes of dstEnd when the match is found

STAGE = (
    [["const", n, 0x41] for n in (0, 3, 4, 127, 128, 191, 192, 193, 4097, 4159)]
    + [["period", n, 7, 3] for n in (128, 191, 193, 4097)]
    + [["period", 5000, 8, 5], ["period", 4159, 9, 1], ["const", 5000, 0xFC], ["text", 4097, 10], ["text", 65599, 11]]
    + [_match(63), _match(64), _match(64 + 253), _match(64 + 254), _match(64 + 2 * 254 + 1), _match(100000)]
    + [_match(203, 0), _match(200, 0), _match(50, 0, [["z", 0x41, 600]]), _match(207, 3)]
    + [_mixed_after_match(1), _mixed_after_match(2), _mixed_after_match(3), _mixed_after_start(), _back_to_back()]
    + [["seq", 4300, 30, [["x", "00010203fcfc41fc"], ["z", 0x41, 3000], ["F", 192, 30], ["z", 0x42, 1050], ["F", 50, 40]]],
       ["seq", 2230, 31, [["z", 0x41, 2000], ["F", 200, 50], ["x", "fcfcfc"], ["r", 27]]],
       ["rnd", 4096, 40], ["rnd", 70001, 41],
       ["sym", 4096, 42, "41fc"], ["sym", 4097, 43, "41fc"], ["sym", 4098, 44, "41fc"], ["sym", 5003, 45, "41fcfc"],
       _fe_run_refused(FE_RUN_FL)]
)
SHORT_CAP = ["text", 4097, 10]           # also run with a destination one byte below the bound (refused, LZCodec.cpp:788)

# inverse inputs that are no LZP output: random bytes, and bytes over the symbols the decoder treats specially
INVERSE = [["rnd", 300, 50], ["rnd", 5000, 51], ["sym", 300, 52, "41fcfeff00"], ["sym", 2000, 53, "41fcfeff00"], ["sym", 700, 54, "4142fc"],
           ["sym", 1500, 55, "41fcff"], ["sym", 64, 56, "41fc05"], ["sym", 3, 57, "41"], ["sym", 4, 58, "41"], ["sym", 900, 59, "41fcfe01"]]
# stage records whose reference output is cut at every position class
CUT_FROM = [_match(64 + 2 * 254 + 1), ["period", 5000, 8, 5], ["text", 4097, 10],
            ["seq", 4300, 30, [["x", "00010203fcfc41fc"], ["z", 0x41, 3000], ["F", 192, 30], ["z", 0x42, 1050], ["F", 50, 40]]]]

STREAM_BS = 65536
STREAM = ["concat", 7 * 65536 + 10, 0, [["text", 65536, 60], ["rnd", 65536, 61], ["const", 65536, 0x20], ["period", 65536, 62, 5],
                                         ["text", 65536, 63], ["text", 65536, 63], ["sym", 65536, 64, "41fc42"], ["rnd", 10, 65]]]
STREAM_CHAINS = [("LZP", "HUFFMAN", 0), ("LZP+BWT+MTFT+ZRLT", "ANS0", 32), ("BWT+LZP", "NONE", 0), ("LZP+LZX", "ANS1", 0)]
HOSTED = [("TEXT+LZP+BWT+RANK+ZRLT", "ANS0", 65536, 0, ["concat", 3 * 65536 + 500, 0, [["text", 3 * 65536 + 500, 70]]])]
CLI = ["concat", 300007, 0, [["text", 200000, 80], ["rnd", 30000, 81], ["period", 70007, 82, 5]]]
