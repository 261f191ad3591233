"""Inputs of the CM coder's tests (entropy id 6), shared by tools/make_cm_golden.py and the tests. An input is a recipe list."""
import vectors


def make(r):
    kind = r[0]
    if kind == "pairs":               # abab...: c1 != c2 at every byte, runMask stays off
        return bytes([r[2], r[3]]) * (r[1] // 2)
    if kind == "dbl":                 # aabbccdd...: runMask on at every second byte
        return bytes(v for i in range(r[1] // 2) for v in ((i * 29 + 5) & 255,) * 2)
    if kind == "adversary":           # every bit the one the predictor rates less likely
        import cm_model
        return cm_model.adversary(r[1])
    if kind == "cat":                 # pieces back to back
        return b"".join(make(p) for p in r[1:])
    return vectors.make(tuple(r))


LENGTHS = [1, 2, 63, 64, 65, 127, 4097]          # copy blocks, around the 64 bytes below which a chunk is still "64 long", tiles

# random bytes whose payload takes a var-int of 1, 2 and 3 bytes (below 128, from 128, from 16,384: test_cm_model.py checks the sizes)
VARINT = [["rand", 100, 11], ["rand", 300, 12], ["rand", 17000, 13]]

ADVERSARY = ["adversary", 8192]

# (name, recipe, block size, checksum bits): one stream each of `kanzi -c -t NONE -e CM -b SIZE -j 1`
STREAMS = (
    [("len%d" % n, ["geom", n, 100 + i, 30], 1 << 20, 0) for i, n in enumerate(LENGTHS)]
    + [("varint%d" % (i + 1), r, 1 << 20, 0) for i, r in enumerate(VARINT)]
    + [
        ("zeros", ["const", 6000, 0], 1 << 20, 0),                # counters and splits at their low end
        ("ones", ["const", 6000, 255], 1 << 20, 0),               # ... and at their high end (cell 16 of counter2)
        ("pairs", ["pairs", 3000, 0x41, 0xBE], 1 << 20, 0),
        ("doubles", ["dbl", 3000], 1 << 20, 0),
        ("ramp", ["ramp", 2048], 1 << 20, 0),                     # every row of both tables
        ("random", ["rand", 4097, 9], 1 << 20, 0),
        ("text", ["text", 20000, 4], 1 << 20, 0),
        ("adversary", ADVERSARY, 1 << 20, 0),
        ("blocks_x32", ["cat", ["text", 9000, 6], ["rand", 3000, 8], ["ramp", 7]], 4096, 32),
        ("blocks_x64", ["cat", ["geom", 7000, 9, 10], ["const", 3000, 7], ["ramp", 11]], 2048, 64),
    ]
)

# whole chains in front of the coder; the last one runs TEXT and UTF on the host (TEXT in its variant 1, which CM selects)
CHAINS = [
    ("BWT+RANK+ZRLT", ["mixed", 40000, 2], 1 << 15, 0),
    ("BWT+MTFT+ZRLT", ["text", 30000, 3], 1 << 14, 32),
    ("LZP", ["cat", ["text", 20000, 5], ["text", 20000, 5]], 1 << 16, 0),
]
HOSTED = [
    ("TEXT+UTF+BWT+LZP", ["text", 60000, 3], 1 << 16, 0),
]
