"""Inputs of the MM (FSDCodec) tests, rebuilt from short recipes: tests/golden/mm.json stores the recipes and what the reference computed
from them (tools/make_mm_golden.py), the tests rebuild the bytes. Generators shared with the PACK tests come from pack_cases."""
import numpy as np

import pack_cases


def max_encoded(n):
    """FSDCodec::getMaxEncodedLength"""
    return n + (64 if n < 1024 else n >> 4)


def walk(n, seed, dist, p):
    """A byte random walk (steps -3 .. 3, a jump of +160 with probability p), interleaved over `dist` classes."""
    r = np.random.default_rng(seed)
    m = (n + dist - 1) // dist
    steps = r.integers(-3, 4, size=(m, dist)) + 160 * (r.random((m, dist)) < p)
    steps[0] += 100
    return (np.cumsum(steps, axis=0) & 255).astype(np.uint8).reshape(-1)[:n].tobytes()


def make(recipe):
    """Bytes of a recipe: [kind, size, seed, ...]; kinds this file does not know go to pack_cases.make."""
    kind, n, seed = recipe[0], recipe[1], recipe[2]
    if kind == "walk":
        return walk(n, seed, recipe[3], recipe[4])
    if kind == "overflow":
        # tenths 2, 3, 6 and 7 alternate 0 / 255: none of them is sampled by the detection, all of them are escapes
        d = bytearray(walk(n, seed, recipe[3], 0.0))
        t = n // 10
        alt = (np.arange(n) & 1).astype(np.uint8) * 255
        for k in (2, 3, 6, 7):
            d[k * t:(k + 1) * t] = alt[k * t:(k + 1) * t].tobytes()
        return bytes(d)
    if kind == "finalfail":
        # tenths 1, 5 and 9 (all the detection samples) hold a walk inside a band of 32 values; tenths 2, 4 and 6 hold noise: tenth 4 makes
        # the large-delta sample choose XOR coding (no overflow), tenths 2 and 6 are what the final check reads from the output
        r = np.random.default_rng(seed)
        band = 100 + np.abs((np.cumsum(r.integers(-3, 4, size=n)) % 62) - 31)
        d = bytearray(band.astype(np.uint8).tobytes())
        t = n // 10
        noise = r.integers(0, 256, n, dtype=np.uint8).tobytes()
        for k in (2, 4, 6):
            d[k * t:(k + 1) * t] = noise[k * t:(k + 1) * t]
        return bytes(d)
    if kind == "magic":
        return (bytes.fromhex(recipe[3]) + make(recipe[4]))[:n]
    if kind == "concat":
        return b"".join(make(r) for r in recipe[3])
    if kind == "mmhdr":
        # an inverse input: mode, dist, then the payload of recipe[5] (a recipe, runs [byte, count, byte, count, ...],
        # or ["rep", runs, runs, times]: the first runs once, the second `times` times)
        body = recipe[5]
        def runs(v):
            return b"".join(bytes([v[i]]) * v[i + 1] for i in range(0, len(v), 2))
        if body and body[0] == "rep":
            pay = runs(body[1]) + runs(body[2]) * body[3]
        elif body and isinstance(body[0], int):
            pay = runs(body)
        else:
            pay = make(body)
        return (bytes([recipe[3], recipe[4]]) + pay)[:n]
    return pack_cases.make(recipe)


STAGE = [
    ["wav", 1 << 20, 60], ["bmp", 1 << 20, 61],
    ["walk", 1700000, 59, 3, 0.01], ["walk", 300000, 62, 1, 0.01], ["walk", 300001, 63, 3, 0.02], ["walk", 262147, 64, 8, 0.01], ["walk", 100003, 65, 16, 0.015],
    ["walk", 200000, 66, 2, 0.1], ["walk", 4096, 67, 4, 0.01], ["walk", 4097, 68, 1, 0.01], ["walk", 8191, 69, 3, 0.01],
    ["walk", 12289, 70, 1, 0.0], ["walk", 1024, 71, 1, 0.01], ["walk", 1023, 72, 1, 0.01], ["walk", 1033, 73, 2, 0.01],
    ["overflow", 200000, 74, 1], ["overflow", 65536, 75, 3], ["finalfail", 200000, 82], ["finalfail", 50001, 83],
    ["text", 100000, 76], ["alpha", 50000, 77, 4], ["random", 50000, 78],
    ["magic", 100000, 0, "89504e47", ["walk", 100000, 79, 1, 0.01]], ["magic", 100000, 0, "50350a", ["walk", 100000, 80, 1, 0.01]],
    ["magic", 100000, 0, "424d", ["walk", 100000, 81, 3, 0.01]],
]

# inverse inputs: arbitrary bytes, every guard, each distance in both modes, runs of 255 of odd and even length, a dangling escape,
# all-escape input
_ESC = [255, 1, 7, 1]
INVERSE = [
    ["random", 3000, 90], ["random", 3, 91], ["mmhdr", 3, 0, 0, 1, [5, 1]], ["mmhdr", 4, 0, 0, 1, [5, 2]],
    ["mmhdr", 100, 0, 0, 0, ["random", 98, 92]], ["mmhdr", 100, 0, 0, 5, ["random", 98, 93]], ["mmhdr", 100, 0, 1, 17, ["random", 98, 94]],
    ["mmhdr", 100, 0, 2, 4, ["random", 98, 95]], ["mmhdr", 9, 0, 0, 8, ["random", 7, 96]], ["mmhdr", 10, 0, 0, 8, ["random", 8, 97]],
    ["mmhdr", 18, 0, 1, 16, ["random", 16, 98]], ["mmhdr", 17, 0, 1, 16, ["random", 15, 99]],
] + [["mmhdr", 20000 + d, 0, m, d, ["random", 20000, 100 + d + 20 * m]] for m in (0, 1) for d in (1, 2, 3, 4, 8, 16)] + [
    ["mmhdr", 5000, 0, 0, 1, ["walk", 5000, 130, 1, 0.0]], ["mmhdr", 30000, 0, 0, 3, ["alpha", 30000, 131, 9]],
    ["mmhdr", 30000, 0, 1, 3, ["walk", 30000, 132, 3, 0.0]],
    ["mmhdr", 40, 0, 0, 1, [9, 3, 255, 3, 8, 4]], ["mmhdr", 40, 0, 0, 1, [9, 3, 255, 4, 8, 4]], ["mmhdr", 40, 0, 0, 2, [9, 3, 255, 5, 8, 1]],
    ["mmhdr", 40, 0, 0, 1, [9, 3, 255, 1]], ["mmhdr", 40, 0, 0, 1, [9, 3, 255, 2]], ["mmhdr", 40, 0, 0, 1, [9, 1, 255, 4001, 3, 2]],
    ["mmhdr", 9001, 0, 0, 1, [9, 1, 255, 8998]], ["mmhdr", 9000, 0, 0, 1, [9, 1, 255, 8997]],
    ["mmhdr", 13003, 0, 0, 1, [9, 1, 255, 9000, 8, 4000]], ["mmhdr", 13004, 0, 0, 2, [9, 2, 255, 9001, 8, 4000]], ["mmhdr", 20003, 0, 0, 4, [255, 20001]],
    ["mmhdr", 20002, 0, 0, 1, ["rep", [9, 1], _ESC, 5000]], ["mmhdr", 30003, 0, 0, 3, ["rep", [1, 1, 2, 1, 3, 1], _ESC, 7500]],
    ["mmhdr", 20018, 0, 0, 16, ["rep", [0, 16], [255, 1, 200, 1], 5000]],
]

# reference forward outputs cut short: [recipe, length]
TRUNCATED = [
    [["walk", 300001, 63, 3, 0.02], 150000], [["walk", 300001, 63, 3, 0.02], 5], [["walk", 300001, 63, 3, 0.02], 4],
    [["walk", 300000, 62, 1, 0.01], 3], [["wav", 1 << 20, 60], 70000], [["wav", 1 << 20, 60], 6], [["bmp", 1 << 20, 61], 500001],
]

# one batch: WAV, walks, text, DNA-like, the overflow block, magic-prefixed blocks, a short tail
STREAM_BS = 1 << 18
STREAM = ["concat", 0, 0, [["wav", STREAM_BS, 140], ["walk", STREAM_BS, 141, 3, 0.01], ["text", STREAM_BS, 142], ["alpha", STREAM_BS, 143, 4],
                           ["overflow", STREAM_BS, 144, 1], ["magic", STREAM_BS, 0, "89504e47", ["walk", STREAM_BS, 145, 1, 0.01]],
                           ["magic", STREAM_BS, 0, "50350a", ["walk", STREAM_BS, 146, 2, 0.01]], ["walk", STREAM_BS, 147, 16, 0.1],
                           ["walk", 5000, 148, 1, 0.01]]]
STREAM_CHAINS = [("MM", "HUFFMAN"), ("MM+PACK", "HUFFMAN"), ("PACK+MM", "NONE"), ("MM+RLT", "NONE"), ("MM+BWT+MTFT+ZRLT", "ANS0")]

# a whole .knz through the host mirror: TEXT / UTF on the host, PACK and MM on the device
HOSTED = [("TEXT+UTF+PACK+MM", "HUFFMAN", 1 << 18, 0,
           ["concat", 0, 0, [["text", 1 << 18, 150], ["walk", 1 << 18, 151, 3, 0.01], ["wav", 1 << 18, 152], ["alpha", 70000, 153, 4]]])]
