"""Inputs of the TPAQ / TPAQX coders' tests (entropy ids 7 and 9), shared by tools/make_tpaq_golden.py and the tests. An input is a
recipe list; every record is taken for both coders."""
import vectors

CODERS = ("TPAQ", "TPAQX")
EXTRA = {"TPAQ": 0, "TPAQX": 1}
ENTROPY_ID = {"TPAQ": 7, "TPAQX": 9}


def make(r):
    kind = r[0]
    if kind == "pairs":               # abab...
        return bytes([r[2], r[3]]) * (r[1] // 2)
    if kind == "cat":                 # pieces back to back
        return b"".join(make(p) for p in r[1:])
    if kind == "hibit":               # random bytes, r[3] percent of them with the top bit set (what _binCount counts)
        import numpy as np
        g = np.random.default_rng(r[2])
        v = g.integers(0, 128, r[1], dtype=np.uint8) | ((g.integers(0, 100, r[1]) < r[3]).astype(np.uint8) << 7)
        return v.tobytes()
    return vectors.make(tuple(r))


LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 4097]          # copy blocks (up to 15), the first coded length, around 64, tiles

# the same 3,000 bytes of text three times with other bytes between: the match model starts, reaches its cap of 88, and is cleared by
# the first bit it mispredicts (at the end of every copy)
REPEATS = ["cat", ["text", 3000, 4], ["text", 3000, 4], ["rand", 500, 3], ["text", 3000, 4], ["text", 2500, 7]]
# 30 % of the bytes with the top bit set: _binCount stays at or above pos >> 2 (the "mostly binary" contexts and the second SSE rule)
BINARY = ["hibit", 5000, 21, 30]
# text (count 0), then half the bytes high -- _binCount passes pos >> 3 after about 1,000 and pos >> 2 after about 3,000 of them -- then
# text again until both fall back
CROSSING = ["cat", ["text", 3000, 9], ["hibit", 5000, 22, 50], ["text", 8000, 10]]

MIB = 1 << 20
# (name, recipe, block size, checksum bits): one stream per coder of `kanzi -c -t NONE -e CODER -b SIZE -j 1`
STREAMS = (
    [("len%d" % n, ["geom", n, 100 + i, 30], MIB, 0) for i, n in enumerate(LENGTHS)]
    + [
        ("const", ["const", 3000, 0xAA], MIB, 0),
        ("ramp", ["ramp", 2048], MIB, 0),
        ("random", ["rand", 4097, 9], MIB, 0),
        ("random8k", ["rand", 8000, 13], MIB, 0),              # above knz_hip_encode_bound and its fixed slack when the first tier is lowered to n / 4
        ("pairs", ["pairs", 3000, 0x41, 0xBE], MIB, 0),
        ("repeats", REPEATS, MIB, 0),
        ("binary", BINARY, MIB, 0),
        ("crossing", CROSSING, MIB, 0),
        # every tier of the states table (below 1 MiB, from 1, 4, 16 and 64 MiB) and masks that are not 2^k - 1 (10000)
        ("bs1024", ["text", 6000, 11], 1024, 0),              # six blocks
        ("bs4096", ["mixed", 9000, 3], 4096, 0),
        ("bs10000", ["cat", ["text", 6000, 12], ["text", 6000, 12], ["hibit", 3000, 23, 40], ["text", 5000, 12]], 10000, 0),
        ("bs4m", ["mixed", 6000, 4], 4 * MIB, 0),
        ("bs16m", ["mixed", 6000, 5], 16 * MIB, 0),
        ("bs64m", ["mixed", 6000, 6], 64 * MIB, 0),
        ("blocks_x32", ["cat", ["text", 5000, 6], ["rand", 2000, 8], ["ramp", 7]], 4096, 32),
        ("blocks_x64", ["cat", ["geom", 4000, 9, 10], ["const", 2000, 7], ["ramp", 11]], 2048, 64),
    ]
)

# whole chains in front of the coder; the HOSTED ones run TEXT on the host (in its variant 1, which these coders select)
CHAINS = [
    ("RLT", ["runs", 40, 300], 1 << 14, 0),
    ("BWT+RANK+ZRLT", ["mixed", 30000, 2], 1 << 12, 0),      # eight blocks: the decoder runs them in three lanes
    ("LZP", ["cat", ["text", 12000, 5], ["text", 12000, 5]], 1 << 15, 32),
]
HOSTED = [
    ("TEXT+UTF", ["text", 20000, 3], 1 << 15, 0),
    ("TEXT+UTF+BWT+RANK+ZRLT", ["text", 30000, 8], 1 << 15, 0),
]
