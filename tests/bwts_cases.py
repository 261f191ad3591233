"""Inputs of the BWTS tests, rebuilt from short recipes: tests/golden/bwts.json stores the recipes and what the reference computed
from them (tools/make_bwts_golden.py), the tests rebuild the bytes."""
import numpy as np

import knzlib


def pi_digits(n):
    """'3.' and the first n decimals of pi (Machin's formula in integers)."""
    def arctan_inv(x, one):
        total, term, k, sign = 0, one // x, 1, 1
        while term:
            total += sign * (term // k)
            term //= x * x
            k += 2
            sign = -sign
        return total
    one = 10 ** (n + 10)
    pi = 4 * (4 * arctan_inv(5, one) - arctan_inv(239, one)) // 10 ** 10
    s = str(pi)
    return (s[0] + "." + s[1:n + 1]).encode()


SIXMIXED = b"SIX.MIXED.PIXIES.SIFT.SIXTY.PIXIE.DUST.BOXES"


def make(recipe):
    """Bytes of a recipe: [kind, size, seed] (or [kind] for the fixed strings)."""
    kind = recipe[0]
    n = recipe[1] if len(recipe) > 1 else 0
    seed = recipe[2] if len(recipe) > 2 else 0
    c = knzlib.corpus()
    if kind == "mississippi":
        return b"mississippi"
    if kind == "pi":
        return pi_digits(n)
    if kind == "sixmixed":
        return SIXMIXED
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "ab_random":
        return np.random.default_rng(seed).integers(97, 99, n, dtype=np.uint8).tobytes()
    if kind == "equal":
        return bytes([seed & 255]) * n
    if kind == "decreasing":
        return bytes((255 - (np.arange(n) % 256)).astype(np.uint8))
    if kind == "abab":
        return (b"ab" * (n // 2 + 1))[:n]
    if kind == "akb":
        return b"a" * (n - 1) + b"b"
    if kind == "text":
        return c.text(n, seed)
    if kind == "mixed":
        return c.mixed(n, seed)
    if kind == "zeros":
        rng = np.random.default_rng(seed)
        z = bytearray(n)
        for p in rng.integers(0, n, max(1, n // 4000)):
            z[int(p)] = int(rng.integers(1, 256))
        return bytes(z)
    if kind == "periodic":
        return c.periodic(n, seed, 7)
    raise ValueError(kind)


# per-stage cases (small enough for the emulator)
STAGE = [
    ["mississippi"], ["pi", 50], ["pi", 2000], ["sixmixed"],
    ["random", 0, 0], ["random", 1, 1], ["random", 2, 2], ["abab", 2],
    ["equal", 1000, 97], ["equal", 4096, 0], ["decreasing", 3000], ["abab", 2000], ["abab", 2001], ["akb", 3000],
    ["random", 5000, 3], ["ab_random", 4000, 4], ["text", 20000, 5], ["zeros", 24000, 6], ["periodic", 6000, 7], ["mixed", 30000, 8],
]

# blocks that are only read as BWTS output (every byte string is one): their inverse is compared with the reference's
INVERSE = [["random", 7000, 11], ["ab_random", 3000, 12], ["text", 9000, 13], ["equal", 500, 5], ["decreasing", 700], ["abab", 999]]

# streams: (chain, entropy, block size, checksum bits, recipe)
STREAMS = [
    ("BWTS+MTFT+ZRLT", "ANS0", 4 << 20, 0, ["mixed", (9 << 20) + 12345, 2]),
    ("BWTS+SRT+ZRLT", "FPAQ", 1 << 20, 0, ["text", (3 << 20) + 777, 3]),
    ("TEXT+UTF+BWTS+RANK+ZRLT", "ANS0", 1 << 20, 0, ["text", (2 << 20) + 4321, 4]),
    ("BWTS+MTFT+ZRLT", "HUFFMAN", 1 << 20, 32, ["mixed", (2 << 20) + 99, 5]),
    ("BWTS", "NONE", 65536, 0, ["mixed", 5 * 65536 + 1001, 6]),
]

# one large single-block round trip
BIG = ["mixed", 256 << 20, 9]

# a stream with the original size in its header, decoded in block ranges and by the sharded path
RANGED = ("BWTS+MTFT+ZRLT", "ANS0", 262144, 0, ["mixed", 11 * 262144 + 5555, 10])
