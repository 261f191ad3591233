"""Inputs of the PACK (AliasCodec) tests, rebuilt from short recipes: tests/golden/pack.json stores the recipes and what the reference
computed from them (tools/make_pack_golden.py), the tests rebuild the bytes."""
import math

import numpy as np


def _rng(seed):
    return np.random.default_rng(seed)


def text(n, seed):
    words = [b"the", b"of", b"and", b"compression", b"block", b"device", b"a", b"to", b"in", b"stream", b"alias", b"pair"]
    r = _rng(seed)
    out = bytearray()
    while len(out) < n:
        out += words[int(r.integers(len(words)))] + (b". " if r.random() < 0.1 else b" ")
    return bytes(out[:n])


def alphabet(n, k, seed):
    """n bytes drawn from k symbols (skewed so that some pairs dominate)."""
    r = _rng(seed)
    head = b"ACGT" + bytes(range(97, 97 + 26)) + bytes(range(48, 58))
    syms = np.frombuffer(head + bytes(c for c in range(256) if c not in head), dtype=np.uint8)[:k]
    p = np.arange(k, 0, -1, dtype=np.float64)
    return syms[r.choice(k, size=n, p=p / p.sum())].tobytes()


def wav(n, seed):
    """RIFF/WAVE 16-bit stereo: a tone with noise."""
    r = _rng(seed)
    frames = max(0, (n - 44) // 4)
    t = np.arange(frames)
    left = (8000 * np.sin(2 * math.pi * 440 * t / 44100) + r.normal(0, 200, frames)).astype("<i2")
    right = (6000 * np.sin(2 * math.pi * 660 * t / 44100) + r.normal(0, 200, frames)).astype("<i2")
    pcm = np.stack([left, right], axis=1).tobytes()
    hdr = b"RIFF" + (36 + len(pcm)).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + bytes([1, 0, 2, 0]) + \
        (44100).to_bytes(4, "little") + (44100 * 4).to_bytes(4, "little") + bytes([4, 0, 16, 0]) + b"data" + len(pcm).to_bytes(4, "little")
    return (hdr + pcm + bytes(n))[:n]


def bmp(n, seed):
    """24-bit BMP with a gradient."""
    w = 256
    h = max(1, (n - 54) // (3 * w) + 1)
    y, x = np.mgrid[0:h, 0:w]
    px = np.stack([(x + seed) % 256, y % 256, (x + y) % 256], axis=2).astype(np.uint8).tobytes()
    hdr = b"BM" + (54 + len(px)).to_bytes(4, "little") + bytes(4) + (54).to_bytes(4, "little") + (40).to_bytes(4, "little") + \
        w.to_bytes(4, "little") + h.to_bytes(4, "little") + bytes([1, 0, 24, 0]) + bytes(24)
    return (hdr + px)[:n]


def make(recipe):
    """Bytes of a recipe: [kind, size, seed, ...]."""
    kind, n, seed = recipe[0], recipe[1], recipe[2]
    if kind == "one":
        return bytes([seed & 255]) * n
    if kind == "alpha":
        return alphabet(n, recipe[3], seed)
    if kind == "text":
        return text(n, seed)
    if kind == "phantom":
        # the first byte makes (0, src[0]) one of the counted pairs: a zero byte is otherwise absent
        d = bytearray(text(n, seed))
        d[0] = ord("e")
        return bytes(d)
    if kind == "random":
        return _rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "random16":
        # 16 bytes values absent: the minimum n0 of the digram mode, savings too low
        return (_rng(seed).integers(16, 256, n, dtype=np.uint8)).tobytes()
    if kind == "wav":
        return wav(n, seed)
    if kind == "bmp":
        return bmp(n, seed)
    if kind == "hdr":
        # random bytes with a few header bytes set: inverse inputs that pass the header guards
        d = bytearray(make(["random", n, seed]))
        for pos, val in recipe[3]:
            d[pos] = val
        return bytes(d)
    if kind == "magic":
        # a magic number in front of a payload PACK would pack: only the data type preset makes it refuse
        return (bytes.fromhex(recipe[3]) + make(recipe[4]))[:n]
    if kind == "truncate":
        return make(recipe[3])[:n]
    if kind == "concat":
        return b"".join(make(r) for r in recipe[3])
    if kind == "onehdr":
        # a one-symbol header with a chosen size field, random bytes behind it
        d = bytearray(make(["random", n, seed]))
        d[0] = 255
        d[2:6] = int(recipe[3]).to_bytes(4, "little")
        return bytes(d)
    raise ValueError(kind)


def overwrite(fwd, seed, k):
    """A forward output with k of its first 64 bytes overwritten (the "overwrite" recipes of DAMAGED: [kind, 0, seed, source recipe, k])."""
    r = _rng(seed)
    d = bytearray(fwd)
    for _ in range(k):
        d[int(r.integers(0, min(64, len(d))))] = int(r.integers(0, 256))
    return bytes(d)


STAGE = [
    ["one", 5000, 65], ["one", 1024, 0],
    ["alpha", 4097, 1, 2], ["alpha", 4098, 2, 3], ["alpha", 4099, 3, 4], ["alpha", 8192, 4, 4],
    ["alpha", 5001, 5, 5], ["alpha", 5002, 6, 16], ["alpha", 70001, 7, 12],
    ["text", 100001, 8], ["text", 100000, 9], ["text", 1 << 20, 10], ["phantom", 65537, 11],
    ["alpha", 300000, 12, 40],
    ["text", 1023, 13], ["random", 50000, 14], ["random16", 50000, 15], ["alpha", 200000, 16, 200],
    # more than 256 chunks of 4,096 parse positions, so that k_pk_f_parse_scan turns its loop twice and carries the token count and the
    # state over: n - 1 = 256 * 4096 + 1 and + 2 (the parse stops on the last byte in one and not in the other), one chunk more; and
    # forward outputs above 256 chunks, so that k_pk_i_scan carries its offset over: 40 symbols, text, and a block of 4 MiB + 3
    ["text", 1048578, 60], ["text", 1048579, 60], ["text", 1052678, 61],
    ["alpha", 1500000, 62, 40], ["text", 2200001, 63], ["alpha", (4 << 20) + 3, 64, 100],
]
LARGE = 1 << 20         # records above this are the ones added for the loops over the chunk table

# reference forward outputs cut short (the inverse reads them as they are): [recipe, length]
TRUNCATED = [
    [["text", 100001, 8], 2000], [["text", 100001, 8], 300], [["text", 100001, 8], 1], [["phantom", 65537, 11], 32977],
    [["alpha", 4099, 3, 4], 40], [["alpha", 4099, 3, 4], 5], [["alpha", 4099, 3, 4], 6], [["alpha", 5002, 6, 16], 17],
    [["alpha", 5002, 6, 16], 18], [["one", 5000, 65], 5], [["one", 5000, 65], 2],
]

INVERSE = [
    ["random", 3000, 20], ["random", 17, 21], ["truncate", 2000, 0, ["text", 100001, 8]],
    ["truncate", 40, 0, ["alpha", 4099, 3, 4]], ["truncate", 5, 0, ["one", 5000, 65]],
    # header guards: 2 + 3 * n0 beyond the end, adjust > 1, one symbol with count < 6 and a negative size,
    # 1 + n + 1 beyond count, adjust >= 4 (2-bit and 4-bit), adjust bytes beyond count
    ["hdr", 50, 40, [[0, 20], [1, 0]]], ["hdr", 62, 41, [[0, 20], [1, 1]]], ["hdr", 500, 42, [[0, 20], [1, 2]]],
    ["hdr", 5, 43, [[0, 255]]], ["hdr", 16, 44, [[0, 255], [5, 200]]], ["hdr", 6, 45, [[0, 254]]],
    ["hdr", 100, 46, [[0, 252], [5, 4]]], ["hdr", 100, 47, [[0, 244], [13, 7]]], ["hdr", 8, 48, [[0, 254], [3, 3]]],
    ["hdr", 19, 49, [[0, 240], [17, 1]]], ["hdr", 18, 50, [[0, 240], [17, 1]]],
    ["hdr", 5000, 22, [[0, 20], [1, 0]]], ["hdr", 5001, 23, [[0, 200], [1, 1]]], ["hdr", 3000, 24, [[0, 250], [7, 1]]],
    ["hdr", 3001, 25, [[0, 253], [4, 3]]], ["hdr", 64, 26, [[0, 255], [2, 100], [3, 0], [4, 0], [5, 0]]],
]

# damaged inverse inputs (at most 100). Header-shaped random bytes: every mode's first byte with the adjust byte of that mode (src[1] in
# the digram mode, src[1 + n] behind the n symbols of a packing mode) at 0 to 5; one-symbol headers by their size field; the reference's
# forward outputs with 1 to 4 of their first 64 bytes overwritten (the test takes the forward output from the emulated kernels, whose
# bytes test 1 has compared, and applies overwrite())
def _damaged():
    out = []
    seed = 300
    for n0 in (15, 16, 17, 100, 239, 240, 243, 244, 251, 252, 254):
        pos = 1 if n0 < 240 else 1 + 256 - n0
        for adjust in range(6):
            # (two lengths above a chunk of 4,096 payload bytes among them)
            out.append(["hdr", 9001 if adjust == 1 and n0 in (100, 244) else 800 + (seed * 131) % 1500, seed, [[0, n0], [pos, adjust]]])
            seed += 1
    for size in (0, 1, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1):
        out.append(["onehdr", 6 + seed % 50, seed, size])
        seed += 1
    srcs = [["alpha", 4099, 3, 4], ["alpha", 5002, 6, 16], ["alpha", 70001, 7, 12], ["text", 100001, 8], ["phantom", 65537, 11],
            ["alpha", 5001, 5, 5], ["one", 5000, 65]]
    for i in range(28):
        out.append(["overwrite", 0, seed, srcs[i % len(srcs)], 1 + i % 4])
        seed += 1
    return out


# one ACGT block under every preset data type: MULTIMEDIA, UTF8, EXE and BIN are refused, UNDEFINED becomes DNA, TEXT stays
PRESET_BLOCK = ["alpha", 8192, 4, 4]
PRESET_TYPES = [2, 3, 7, 8, 0, 1]

DAMAGED = _damaged()
DAMAGED_CAP_MIN = 1 << 17       # room for the one-symbol header of 65,536 bytes


# one batch whose blocks have different data types: text, WAV (MULTIMEDIA preset: PACK refuses), BMP, random, DNA, a short tail
# and blocks that start with a RIFF, BMP, PGM, ELF or PNG magic over text or a small alphabet (MULTIMEDIA, EXE and BIN presets)
STREAM = ["concat", 0, 0, [["text", 1 << 20, 30], ["wav", 1 << 20, 31], ["bmp", 1 << 20, 32], ["random", 1 << 20, 33],
                           ["alpha", 1 << 20, 34, 4], ["alpha", 1 << 20, 35, 12],
                           ["magic", 1 << 20, 0, "52494646", ["text", 1 << 20, 37]], ["magic", 1 << 20, 0, "424d", ["text", 1 << 20, 38]],
                           ["magic", 1 << 20, 0, "50350a", ["alpha", 1 << 20, 39, 12]], ["magic", 1 << 20, 0, "7f454c46", ["text", 1 << 20, 40]],
                           ["magic", 1 << 20, 0, "89504e47", ["alpha", 1 << 20, 41, 3]], ["text", 10, 36]]]
STREAM_BS = 1 << 20
# (RLT refuses the DNA block by the type PACK leaves on it)
STREAM_CHAINS = [("PACK", "HUFFMAN"), ("PACK+BWT+MTFT+ZRLT", "ANS0"), ("PACK+RLT", "NONE"), ("PACK+ZRLT", "ANS1")]

# whole .knz files through the host mirror: TEXT / UTF on the host hand their data type to PACK on the device
HOSTED = [("TEXT+PACK", "HUFFMAN", 1 << 20, 0, ["concat", 0, 0, [["text", 1 << 20, 50], ["alpha", 1 << 20, 51, 4], ["text", 70000, 52]]]),
          ("UTF+PACK+RLT", "NONE", 1 << 20, 32, ["concat", 0, 0, [["alpha", 1 << 20, 53, 4], ["text", 1 << 20, 54]]])]
