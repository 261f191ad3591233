"""Inputs of the RANGE coder's tests (entropy id 4), shared by tools/make_range_golden.py and the tests. An input is a recipe list."""
import numpy as np

import vectors


def make(r):
    kind = r[0]
    if kind == "alpha":               # n bytes drawn evenly from k symbols spread over the byte range
        _, n, seed, k = r
        syms = np.array([(i * 37 + 11) & 255 for i in range(k)], dtype=np.uint8)
        return syms[np.random.default_rng(seed).integers(0, k, n)].tobytes()
    if kind == "mid":                 # a coded chunk, a constant chunk, a coded tail: the decoder steps over a chunk without payload
        _, seed, tail = r
        return make(["alpha", 32768, seed, 256]) + bytes([0x41]) * 32768 + make(["geom", tail, seed + 1, 30])
    if kind == "wide":                # 280 bytes, 255 values: see WIDE
        _, seed = r
        g = np.random.default_rng(seed)
        vals = g.permutation(256)[1:]
        counts = np.ones(255, dtype=np.int64)
        counts[0] += 9; counts[1] += 7; counts[2] += 3; counts[3:9] += 1
        return g.permutation(np.repeat(vals, counts)).astype(np.uint8).tobytes()
    if kind == "cat":                 # pieces back to back
        return b"".join(make(p) for p in r[1:])
    return vectors.make(tuple(r))


# lengths at the log-range steps (2^lr <= n: 8 below 512, 9, 10, 11, 12 from 4,096 on) and around the 32,768-byte chunk
LENGTHS = [1, 2, 255, 256, 1023, 1024, 4095, 4096, 4097, 32767, 32768, 32769, 65541, 3 * 32768 + 5]

# (name, recipe, block size, checksum bits): one stream each of `kanzi -c -t NONE -e RANGE -b SIZE -j 1`
STREAMS = (
    [("len%d" % n, ["geom", n, 100 + i, 30], 1 << 20, 0) for i, n in enumerate(LENGTHS)]
    + [("alpha%d_%d" % (k, n), ["alpha", n, 7 * k, k], 1 << 20, 0) for k in (63, 64, 65) for n in (255, 1024, 4097)]
    + [
        ("one_symbol", ["const", 40000, 65], 1 << 20, 0),
        ("two_symbols", ["twosym", 50000, 5], 1 << 20, 0),
        ("uniform256", ["rand", 65541, 9], 1 << 20, 0),           # also the most 28-bit units a chunk of the cases leaves
        ("ramp256", ["ramp", 256], 1 << 20, 0),                   # n == scale at lr 8: the frequencies are taken as counted
        ("ramp4096", ["ramp", 4096], 1 << 20, 0),
        ("skewed", ["geom", 100001, 3, 70], 1 << 20, 0),
        ("pow_tail", ["pow", 40000, 17, 5, 256], 1 << 20, 0),     # long tail of frequency-1 symbols: the error is spread in rounds
        ("text", ["text", 70000, 4], 1 << 20, 0),
        ("middle_constant", ["mid", 21, 5000], 1 << 20, 0),
        ("underflow", ["rand", 32768, 10], 1 << 20, 0),            # (the seed is set by UNDERFLOW below)
        ("copy_block", ["ramp", 15], 1 << 20, 0),
        ("ramp16", ["ramp", 16], 1 << 20, 0),
        ("blocks", ["cat", ["text", 65536, 2], ["alpha", 65536, 3, 200], ["geom", 12345, 4, 20]], 65536, 0),
        ("blocks_x32", ["cat", ["text", 40000, 6], ["rand", 30000, 8]], 16384, 32),
        ("blocks_x64", ["cat", ["geom", 33000, 9, 10], ["const", 20000, 7], ["ramp", 7]], 32768, 64),
    ]
)

# a chunk of random bytes on which the encoder cuts the range back to the next 2^16 border at least once (found with range_model.Stats
# by tools/make_range_golden.py --find-underflow)
UNDERFLOW = ["rand", 32768, 10]

# A chunk on which the reference's normalisation ends below zero: shorter than 512 bytes (log range 8), 255 values with counts 10, 8, 4,
# six times 2 and 246 times 1. The scaled frequencies sum to 278; five rounds take 12 off the three that exceed 2, and the largest,
# by then 4, gets 4 - 10 = 0xFFFFFFFA (EntropyUtils.cpp:243). The reference writes the chunk and cannot read it; its bytes carry what
# its unmasked writeBits and its 64-bit products leave, which depends on where the chunk lies in the 64-bit words of the block's bit
# stream. Alone (by the seed the wide symbol is the first of the alphabet, whose frequency is not written, or a later one), behind a
# chunk of 32,768 bytes whose length in bits moves it. (Only the last chunk of a block can be this short.)
WIDE = [["wide", s] for s in range(1, 7)] + [["cat", ["geom", 32768, 200 + s, 12 + 9 * s], ["wide", 10 + s]] for s in range(8)]
# (recipe, block size, checksum bits, jobs): the chunk inside a framed stream, behind block headers of different lengths
WIDE_STREAMS = [(["wide", 30], 65536, 0, 1), (["wide", 31], 65536, 32, 2), (["wide", 32], 1024, 64, 1),
                (["cat", ["text", 65536, 8], ["geom", 32768, 211, 25], ["wide", 34]], 65536, 32, 3)]

# whole chains in front of the coder; the last one runs TEXT and UTF on the host
CHAINS = [
    ("BWT+MTFT+ZRLT", ["mixed", 300000, 2], 1 << 18, 0),
    ("RLT", ["cat", ["runs", 9000, 60], ["text", 100000, 3]], 1 << 16, 32),
]
HOSTED = [
    ("TEXT+UTF+BWT+RANK+ZRLT", ["text", 300000, 3], 1 << 18, 0),
]
