"""Inputs of the UTF tests, rebuilt from short recipes: tests/golden/utf.json stores the recipes and what the reference computed from
them (tools/make_utf_golden.py), the tests rebuild the bytes. A recipe is [kind, size, seed, ...]; a stage case is (recipe, data type
the block comes with)."""
import numpy as np

import vectors

CHUNK = 4096           # bytes per workgroup of the device stage (utf.hip: UT_CHUNK), 16 per thread
SCAN_TILE = 256        # chunks per step of the per-block scan over the chunks


def cps(distinct, draws, seed):
    """The code points 0x800.. (three bytes each) twice over, then `draws` of the first 300 of them."""
    rng = np.random.default_rng(seed)
    pts = list(range(0x800, 0x800 + distinct)) * 2 + [0x800 + int(x) for x in rng.integers(0, min(300, distinct), draws)]
    a = np.array(pts, dtype=np.uint32)
    out = np.empty((len(a), 3), dtype=np.uint8)
    out[:, 0] = 0xE0 | (a >> 12)
    out[:, 1] = 0x80 | ((a >> 6) & 0x3F)
    out[:, 2] = 0x80 | (a & 0x3F)
    return out.tobytes()


def utf8(n, seed):
    """n bytes of the utf8 vector (it draws n / 2 + 16 code points of one byte and more, so twice the length is asked for)"""
    return vectors.make(("utf8", 2 * n + 64, seed))[:n]


def make(recipe):
    kind, n, seed = recipe[0], recipe[1], recipe[2]
    if kind == "utf8":
        d = utf8(n, seed)
    elif kind == "cut":              # the utf8 stream with its first recipe[3] bytes cut off
        d = utf8(n + recipe[3], seed)[recipe[3]:]
    elif kind == "bom":
        d = b"\xef\xbb\xbf" + utf8(n - 3, seed)
    elif kind == "ascii":
        d = vectors.make(("text", n, seed))
    elif kind == "rnd":
        d = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    elif kind == "cps":              # [.., distinct, draws], cut to n bytes
        d = cps(recipe[3], recipe[4], seed)[:n]
    elif kind == "plant":            # [.., base recipe, position, hex]
        d = bytearray(make(recipe[3]))
        h = bytes.fromhex(recipe[5])
        d[recipe[4]:recipe[4] + len(h)] = h
        d = bytes(d)
    elif kind == "concat":
        d = b"".join(make(r) for r in recipe[3])
    elif kind == "rep":              # the first recipe[3] bytes of the utf8 stream, repeated
        unit = utf8(recipe[3], seed)
        d = (unit * (n // len(unit) + 1))[:n]
    else:
        raise ValueError(kind)
    assert len(d) == n, (recipe[:3], len(d))
    return d


def _cps(distinct, draws, seed, n=None):
    return ["cps", n if n is not None else 3 * (2 * distinct + draws), seed, distinct, draws]


_BASE = _cps(200, 2000, 20)          # 7,200 bytes of three-byte symbols: position 3 k is a lead byte

STAGE = (
    [(["utf8", n, 1], 0) for n in (0, 1023, 1024, 1025, 4096, 65536 + 77)]
    + [(["cut", 5000, 2, k], 0) for k in range(1, 8)]
    + [(["utf8", n, 3], 0) for n in range(6000, 6005)]
    + [(["bom", 5000, 4], 0), (["utf8", 5000, 5], 1), (["utf8", 5000, 5], 8)]
    + [(["ascii", 4096, 6], 0), (["ascii", 4096, 6], 8)]
    + [(_cps(200, 20000, 10), 0), (_cps(5000, 20000, 11), 0), (_cps(20000, 200000, 12), 0), (_cps(32767, 200000, 13), 0),
       (_cps(32768, 20000, 14), 0), (_cps(40000, 20000, 15), 0)]
    + [(["plant", 7200, 0, _BASE, 300, "c04142"], 0), (["plant", 7200, 0, _BASE, 300, "c04142"], 8),
       (["plant", 7200, 0, _BASE, 302, "41"], 0), (["plant", 7200, 0, _BASE, 302, "41"], 8),
       (["plant", 7200, 0, _BASE, 301, "41"], 8),
       (["rnd", 4096, 30], 8), (["rnd", 4096, 30], 0)]
    # the symbol walk covers [start, count - 4): lengths that put its end at a chunk's end -1, +0, +1, +3 (one chunk, two chunks), with
    # three-byte symbols across every stretch and chunk border, and one block of more than SCAN_TILE chunks
    + [(_cps(100, 3000, 40, CHUNK + 4 + k), 0) for k in (-1, 0, 1, 3)]
    + [(_cps(100, 3000, 41, 2 * CHUNK + 4 + k), 0) for k in (-1, 0, 1, 3)]
    + [(_cps(300, 400000, 42, SCAN_TILE * CHUNK + 4 + 3), 0)]
)
LOSSY = ["plant", 7200, 0, _BASE, 301, "41"]     # taken under type 8, and the reference's inverse does not give it back

# capacity checks stated from UTFCodec.cpp:62 (the reference's sequence gives a stage a buffer of its own when the caller's is short)
CAP_CASE = ["utf8", 4096, 1]

# damage done to the forward output of a stage record (by index into STAGE) before it is decoded
DAMAGE_FROM = [4, 24, 18]            # utf8 4096; 5000 distinct symbols (two-byte aliases); the BOM
DAMAGE = ["cut1", "cutmap", "cutmid", "n0", "hdr1", "alias", "class"]
INVERSE_RND = [["rnd", 300, 50], ["rnd", 5000, 51], ["rnd", 3, 52], ["rnd", 4, 53]]


def damage(out, op):
    d = bytearray(out)
    n = (d[2] << 8) + d[3]
    if op == "cut1":
        return bytes(d[:-1])
    if op == "cutmap":
        return bytes(d[:4 + 3 * (n // 2) + 1])
    if op == "cutmid":
        return bytes(d[:(4 + 3 * n + len(d)) // 2])
    if op == "n0":
        d[2] = d[3] = 0
    elif op == "hdr1":
        d[1] = (d[1] + 1) & 3
    elif op == "alias":              # an alias of 32,767 in the middle of the stream
        at = (4 + 3 * n + len(d)) // 2
        d[at] = d[at + 1] = 0xFF
    elif op == "class":              # size class 3 does not exist (unpack returns 0)
        d[4 + 3 * (n // 2)] = 0x18
    else:
        raise ValueError(op)
    return bytes(d)


# chains over eight blocks of 64 KiB (code points cut at the block borders) and a tail of 10 bytes
STREAM_BS = 65536
STREAM = ["concat", 8 * 65536 + 10, 0, [["utf8", 3 * 65536, 60], ["ascii", 65536, 61], ["rnd", 65536, 62], ["rep", 65536, 63, 3000],
                                         _cps(5000, 11846, 64, 65536), ["utf8", 65536 + 10, 65]]]
STREAM_CHAINS = [("UTF", "NONE", 0), ("UTF+BWT+RANK+ZRLT", "ANS0", 0), ("LZP+UTF+BWT+LZP", "CM", 0), ("UTF+PACK+RLT", "NONE", 32)]
# mixed input: blocks TEXT takes, blocks UTF takes, blocks neither takes
HOSTED_INPUT = ["concat", 6 * 65536 + 500, 0, [["ascii", 2 * 65536, 70], ["utf8", 2 * 65536, 71], ["rnd", 65536, 72], ["ascii", 65536 + 500, 73]]]
HOSTED = [("TEXT+UTF+BWT+RANK+ZRLT", "ANS0", 65536, 0), ("UTF+BWT+SRT+ZRLT", "FPAQ", 65536, 0)]
CLI = ["concat", 300007, 0, [["utf8", 200000, 80], ["rnd", 30000, 81], ["ascii", 70007, 82]]]
CLI_ARGS = ["-t", "LZP+UTF+BWT+RANK+ZRLT", "-e", "ANS0"]
