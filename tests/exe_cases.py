"""Inputs of the EXE tests, rebuilt from short recipes: tests/golden/exe.json stores the recipes and what the reference computed from
them (tools/make_exe_golden.py), the tests rebuild the bytes. A recipe is [kind, size, seed, ...]; a stage case is (recipe, data type
the block comes with, name)."""
import struct

import numpy as np

CHUNK = 4096           # positions per workgroup of the device stage (exe.hip: EX_CHUNK), 16 per thread
SCAN_TILE = 256        # chunks per step of the per-block composition
UNDEFINED, TEXT, MULTIMEDIA, EXE, DNA, BIN = 0, 1, 2, 3, 6, 7
VALUES_AT = 600        # the 256 byte values lie this far in front of the end of a generated block


def max_encoded(n):
    """EXECodec::getMaxEncodedLength"""
    return n + 32 if n <= 256 else n + n // 8


def _all_values():
    """Every byte value once, four to a word whose top byte is 0xC0 or more (no ARM64 branch, no x86 jump in its last byte)"""
    return bytes((k + 64 * j) & 255 for k in range(64) for j in range(4))


def _finish(out, n, origin):
    out = bytearray(out[:n])
    at = origin + ((n - origin - VALUES_AT) & ~3) if n - origin >= VALUES_AT + 256 else None
    if at is not None:
        out[at:at + 256] = _all_values()
    return out


def x86(n, seed, origin=0):
    """Instruction-like bytes of 16 and more (no 9B, E8 or E9) with E8 / E9 / 0F 8x and a rel32 within +-60,000 about every 40 bytes,
    runs of 00 (about 14 % of the bytes) and of FF (about 2 %), the 256 byte values once near the end; the first `origin` bytes are
    plain filler."""
    rng = np.random.default_rng(seed)
    out = bytearray(rng.integers(16, 256, origin, dtype=np.uint8).tobytes())
    plain = np.array([v for v in range(16, 256) if v not in (0x9B, 0xE8, 0xE9)], dtype=np.uint8)
    ops = (b"\xe8", b"\xe9", b"\x0f\x84", b"\x0f\x85", b"\x0f\x8c")
    while len(out) < n:
        r = rng.random()
        if r < 0.24:
            out += bytes(int(rng.integers(8, 40)))
        elif r < 0.28:
            out += b"\xff" * int(rng.integers(4, 20))
        else:
            out += plain[rng.integers(0, len(plain), int(rng.integers(20, 60)))].tobytes()
            out += ops[int(rng.integers(0, len(ops)))] + struct.pack("<i", int(rng.integers(-60000, 60000)))
    return _finish(out, n, origin)


def arm(n, seed, origin=0, below=0):
    """Words from `origin`: 6 % B / BL with a target inside the block (behind its first word), 24 % zero, 6 % FFFFFFFF, the rest random
    and no branch, the 256 byte values once near the end; `below` more branches, right at the start, have targets below address 0."""
    rng = np.random.default_rng(seed)
    head = rng.integers(16, 256, origin, dtype=np.uint8).tobytes()
    nw = (n - origin) // 4
    w = rng.integers(0, 1 << 32, nw, dtype=np.uint64)
    op = w & 0xFC000000
    w = np.where((op == 0x14000000) | (op == 0x94000000), w ^ 0x40000000, w)
    kind = rng.random(nw)
    w = np.where(kind < 0.24, 0, w)
    w = np.where((kind >= 0.24) & (kind < 0.30), 0xFFFFFFFF, w)
    idx = np.arange(nw, dtype=np.int64)
    target = rng.integers(1, max(nw, 2), nw, dtype=np.int64)
    branch = np.where(rng.random(nw) < 0.5, 0x14000000, 0x94000000) | ((target - idx) & 0x03FFFFFF)
    w = np.where((kind >= 0.30) & (kind < 0.36), branch, w)
    for k in range(below):
        w[1 + k] = 0x14000000 | ((-(origin // 4 + 6 + k)) & 0x03FFFFFF)
    body = w.astype("<u4").tobytes()
    tail = rng.integers(16, 256, n - origin - 4 * nw, dtype=np.uint8).tobytes()
    return _finish(head + body + tail, n, origin)


def text(n, seed):
    rng = np.random.default_rng(seed)
    pool = [rng.integers(97, 123, int(rng.integers(2, 10)), dtype=np.uint8).tobytes() for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += pool[int(rng.integers(0, 200))] + (b"\n" if rng.random() < 0.1 else b" ")
    return bytes(out[:n])


def _payload(kind, n, seed, origin):
    if kind == "x86":
        return x86(n, seed, origin)
    if kind == "arm":
        return arm(n, seed, origin)
    if kind == "text":
        return bytearray(text(n, seed))
    if kind == "rnd":
        return bytearray(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes())
    raise ValueError(kind)


def elf(n, seed, payload, arch, bits, little, sections):
    """An ELF header and a section table at 64 (sections: [offset, length, type]) over a payload that starts at the first section"""
    d = _payload(payload, n, seed, sections[0][0] if sections[0][0] < n else 4096)
    e = "<" if little else ">"
    d[0:6] = b"\x7fELF" + bytes([2 if bits == 64 else 1, 1 if little else 2])
    d[6:64] = bytes(58)
    struct.pack_into(e + "H", d, 18, arch)
    if bits == 64:
        struct.pack_into(e + "Q", d, 0x28, 64)
        struct.pack_into(e + "HH", d, 0x3A, 0x40, len(sections))
        for i, (off, ln, typ) in enumerate(sections):
            at = 64 + 0x40 * i
            d[at:at + 0x40] = bytes(0x40)
            struct.pack_into(e + "I", d, at + 4, typ)
            struct.pack_into(e + "QQ", d, at + 0x18, off, ln)
    else:
        struct.pack_into(e + "I", d, 0x20, 64)
        struct.pack_into(e + "HH", d, 0x2E, 0x28, len(sections))
        for i, (off, ln, typ) in enumerate(sections):
            at = 64 + 0x28 * i
            d[at:at + 0x28] = bytes(0x28)
            struct.pack_into(e + "I", d, at + 4, typ)
            struct.pack_into(e + "II", d, at + 0x10, off, ln)
    return d


def pe(n, seed, payload, arch, base, size):
    d = _payload(payload, n, seed, base)
    d[0:64] = b"MZ" + bytes(62)
    struct.pack_into("<i", d, 60, 128)
    d[128:128 + 48] = bytes(48)
    struct.pack_into("<IH", d, 128, 0x00004550, arch)
    struct.pack_into("<i", d, 128 + 28, size)
    struct.pack_into("<i", d, 128 + 44, base)
    return d


def macho64(n, seed, payload, arch, off, size):
    d = _payload(payload, n, seed, off)
    d[0:0x20 + 0x48 + 0x50] = bytes(0x20 + 0x48 + 0x50)
    d[0:4] = b"\xcf\xfa\xed\xfe"
    struct.pack_into("<i", d, 4, arch)
    struct.pack_into("<i", d, 12, 2)
    struct.pack_into("<i", d, 0x10, 2)
    struct.pack_into("<ii", d, 0x20, 0x19, 0x48)                   # a segment that is not __TEXT
    d[0x28:0x2E] = b"__DATA"
    pos = 0x20 + 0x48
    struct.pack_into("<ii", d, pos, 0x19, 0x48 + 0x50)
    d[pos + 8:pos + 14] = b"__TEXT"
    sec = pos + 0x48
    d[sec:sec + 6] = b"__text"
    struct.pack_into("<i", d, sec + 0x28, size)
    struct.pack_into("<q", d, sec + 0x30, off)
    return d


def make(recipe):
    kind, n, seed = recipe[0], recipe[1], recipe[2]
    if kind == "x86":
        d = x86(n, seed)
    elif kind == "arm":
        d = arm(n, seed, 0, recipe[3] if len(recipe) > 3 else 0)
    elif kind == "elf":
        d = elf(n, seed, *recipe[3:])
    elif kind == "pe":
        d = pe(n, seed, *recipe[3:])
    elif kind == "macho64":
        d = macho64(n, seed, *recipe[3:])
    elif kind == "text":
        d = text(n, seed)
    elif kind == "rnd":
        d = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    elif kind == "dna":
        d = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()
    elif kind == "plant":            # [.., base recipe, position (negative: from the end), hex]
        d = bytearray(make(recipe[3]))
        h = bytes.fromhex(recipe[5])
        at = recipe[4] if recipe[4] >= 0 else len(d) + recipe[4]
        d[at:at + len(h)] = h
    elif kind == "esc":              # [.., base recipe, k]: k bytes of the block's first part become 9B
        d = bytearray(make(recipe[3]))
        for at in np.random.default_rng(seed).choice(len(d) - 2 * VALUES_AT, recipe[4], replace=False):
            d[int(at)] = 0x9B
    elif kind == "concat":
        d = b"".join(make(r) for r in recipe[3])
    elif kind == "tile":             # the base recipe repeated to the size
        unit = make(recipe[3])
        d = (unit * (n // len(unit) + 1))[:n]
    else:
        raise ValueError(kind)
    assert len(d) == n, (recipe[:3], len(d))
    return bytes(d)


NOPS = "909090909090"      # six plain bytes: whatever state the parse arrives in, the byte behind them is at an opcode
_X = ["x86", 8192, 3]
_ELF2 = [[4096, 2000, 1], [6096, 2096, 1]]


def _plant(base, at, hexes):
    return ["plant", base[1], 0, base, at, hexes]


# (recipe, data type the block comes with, name)
STAGE = (
    [(["x86", n, 1], UNDEFINED, "x86 %d" % n) for n in (4095, 4096, 4097, 4099, 8192, 65536, 300001)]
    + [(["arm", n, 2], UNDEFINED, "arm %d" % n) for n in (4095, 4096, 4097, 4099, 65536 + 6)]
    + [(["arm", 4096, 2, k], UNDEFINED, "arm %d below 0" % k) for k in (4, 17, 18, 19, 25)]
    + [(["elf", 8192, 4, "x86", 0x3E, 64, True, _ELF2], UNDEFINED, "elf64 x86"),
       (["elf", 8192, 5, "arm", 0xB7, 64, True, _ELF2], UNDEFINED, "elf64 arm"),
       (["elf", 8192, 6, "x86", 0xF3, 64, True, _ELF2], UNDEFINED, "elf64 unknown arch"),
       (["elf", 8192, 7, "x86", 0x3E, 64, True, [[4096, 5000, 1]]], UNDEFINED, "elf64 section beyond the block"),
       (["elf", 8192, 8, "x86", 0x3E, 64, True, [[4096, 256, 1]]], EXE, "elf64 code range of 256"),
       (["elf", 8192, 9, "x86", 0x3E, 64, True, [[4096, 3000, 1], [7096, 5000, 1]]], UNDEFINED, "elf64 good then bad section"),
       (["elf", 8192, 10, "text", 0xF3, 64, True, _ELF2], EXE, "elf magic preset EXE, rejected"),
       (["elf", 8192, 11, "rnd", 0xF3, 64, True, _ELF2], EXE, "elf magic preset EXE, random"),
       (["elf", 8192, 12, "x86", 0x03, 32, True, _ELF2], UNDEFINED, "elf32"),
       (["elf", 8192, 13, "x86", 0x3E, 64, False, _ELF2], UNDEFINED, "elf64 big endian"),
       (["elf", 8192, 14, "arm", 0xB7, 32, False, _ELF2], UNDEFINED, "elf32 big endian arm"),
       (["elf", 8192, 15, "arm", 0xB7, 64, True, [[4098, 2000, 1], [6098, 2090, 1]]], UNDEFINED, "elf64 arm codeStart 4098"),
       (["elf", 8192, 16, "x86", 0x3E, 64, True, [[4096, 2000, 8], [100, 32, 1], [5000, 3000, 1]]], UNDEFINED, "elf64 skipped sections"),
       (["pe", 8192, 17, "x86", 0x014C, 4096, 4000], UNDEFINED, "pe x86"),
       (["pe", 8192, 18, "x86", 0x8664, 4096, 4000], UNDEFINED, "pe amd64 (arch read as a signed 16-bit value)"),
       (["macho64", 8192, 19, "x86", 0x01000007, 4096, 4000], UNDEFINED, "macho64 x86"),
       (["macho64", 8192, 20, "arm", 0x0100000C, 4096, 4000], UNDEFINED, "macho64 arm")]
    + [(_X, dt, "x86 preset %d" % dt) for dt in (TEXT, MULTIMEDIA, EXE, BIN)]
    + [(["rnd", 8192, 21], UNDEFINED, "random"), (["text", 8192, 22], UNDEFINED, "text"), (["dna", 8192, 23], UNDEFINED, "acgt")]
    + [(_plant(_X, -1 - 6, NOPS + "0f"), UNDEFINED, "x86 lone 0f at the end"),
       (_plant(_X, -4 - 6, NOPS + "0f85"), UNDEFINED, "x86 0f 85 4 before the end"),
       (_plant(_X, -5 - 6, NOPS + "0f85"), UNDEFINED, "x86 0f 85 5 before the end"),
       (_plant(_X, -6 - 6, NOPS + "0f85"), UNDEFINED, "x86 0f 85 6 before the end"),
       (_plant(_X, -3 - 6, NOPS + "e8"), UNDEFINED, "x86 e8 3 before the end"),
       (_plant(_X, -4 - 6, NOPS + "e8"), UNDEFINED, "x86 e8 4 before the end"),
       (_plant(_X, -5 - 6, NOPS + "e8"), UNDEFINED, "x86 e8 5 before the end"),
       (_plant(_X, 3000, NOPS + "e8000000ff" + NOPS + "e9000000ff" + NOPS + "0f84000000ff"), UNDEFINED, "x86 rel32 ff000000"),
       (_plant(_X, 3000, NOPS + "9b909b9b0f9b900f9b0f9b9b"), UNDEFINED, "x86 9b at an opcode and behind 0f"),
       (_plant(_X, 3000, NOPS + "0f0f0f0f0f900f38850f3a81900f380f3a0f3838850f0f85" + NOPS), UNDEFINED, "x86 0f runs"),
       (_plant(_X, CHUNK - 3, "e8102030"), UNDEFINED, "x86 jump across a chunk border"),
       (["esc", 65536, 30, ["x86", 65536, 1], 900], UNDEFINED, "x86 900 more 9b"),
       (["esc", 65536, 31, ["x86", 65536, 1], 1400], UNDEFINED, "x86 1400 more 9b"),
       (["x86", SCAN_TILE * CHUNK + 651424, 32], UNDEFINED, "x86 1.7 MB")]
)
REQUIRED = {        # name -> (ok, data type left) the reference must give (tools/make_exe_golden.py asserts it)
    "x86 4095": (0, UNDEFINED), "x86 4096": (1, EXE), "x86 4097": (1, EXE), "x86 4099": (1, EXE), "x86 8192": (1, EXE),
    "x86 65536": (1, EXE), "x86 300001": (1, EXE), "arm 4095": (0, UNDEFINED), "arm 4096": (1, EXE), "arm 4097": (1, EXE),
    "arm 4099": (1, EXE), "arm 4 below 0": (1, EXE), "elf64 x86": (1, EXE), "elf64 arm": (1, EXE), "elf64 unknown arch": (1, EXE),
    "elf64 section beyond the block": (1, EXE), "elf64 code range of 256": (0, EXE), "elf magic preset EXE, rejected": (0, UNDEFINED),
    "elf magic preset EXE, random": (0, BIN), "elf32": (1, EXE), "elf64 big endian": (1, EXE), "elf64 arm codeStart 4098": (1, EXE),
    "pe x86": (1, EXE), "macho64 x86": (1, EXE), "x86 preset 1": (0, TEXT), "x86 preset 2": (0, MULTIMEDIA), "x86 preset 3": (1, EXE),
    "x86 preset 7": (1, EXE), "random": (0, BIN), "text": (0, UNDEFINED), "acgt": (0, DNA), "x86 900 more 9b": (1, EXE),
    "x86 1400 more 9b": (0, UNDEFINED), "x86 1.7 MB": (1, EXE), "x86 rel32 ff000000": (1, EXE),
}

# damage done to the forward output of a stage record (by name) before it is decoded
DAMAGE_FROM = ["x86 8192", "elf64 x86", "arm 4 below 0", "elf64 arm"]
DAMAGE = ["whole", "cuthdr", "cutprefix", "cutmid", "cut1", "cut2", "cut3", "cut4", "end-1", "end+1", "endbig", "startneg", "startbig",
          "mode", "escend", "armhalf"]


def damage(out, op):
    """None where the damage does not apply to the record"""
    d = bytearray(out)
    start, end = struct.unpack_from("<ii", d, 1)
    if op == "whole":
        return bytes(d)
    if op == "cuthdr":
        return bytes(d[:5])
    if op == "cutprefix":
        return bytes(d[:9 + start // 2]) if start else None
    if op == "cutmid":
        return bytes(d[:(9 + start + end) // 2])
    if op in ("cut1", "cut2", "cut3", "cut4"):
        return bytes(d[:end - int(op[3])])
    if op == "end-1":
        struct.pack_into("<i", d, 5, end - 1)
    elif op == "end+1":
        struct.pack_into("<i", d, 5, end + 1)
    elif op == "endbig":
        struct.pack_into("<i", d, 5, len(d) + 1)
    elif op == "startneg":
        struct.pack_into("<i", d, 1, -1)
    elif op == "startbig":
        struct.pack_into("<i", d, 1, end - 8)
    elif op == "mode":
        d[0] ^= 0x60
    elif op == "escend":             # x86: the last byte of the code becomes an escape
        if d[0] != 0x40:
            return None
        d[end - 1] = 0x9B
    elif op == "armhalf":            # ARM64: the code ends behind the first word of the first escape pair
        if d[0] != 0x20:
            return None
        at = next((p for p in range(9 + start, end - 4, 4) if d[p + 3] in (0x14, 0x94) and d[p:p + 3] == b"\0\0\0"), None)
        if at is None:
            return None
        struct.pack_into("<i", d, 5, at + 4)
    else:
        raise ValueError(op)
    return bytes(d)


# 71 blocks of 4,096 bytes (the last one 100) of every kind
RAGGED_BS = 4096
RAGGED = ["concat", 70 * 4096 + 100, 0,
          [[("x86", "arm", "text", "rnd", "x86", "dna", "arm")[i % 7], 4096, 100 + i] for i in range(70)] + [["text", 100, 99]]]
# 64 KiB blocks of x86, text, ARM64, an ELF block, x86 again and a tail of 1,000 bytes
STREAM_BS = 65536
STREAM = ["concat", 5 * 65536 + 1000, 0, [["x86", 65536, 40], ["text", 65536, 41], ["arm", 65536, 42],
                                           ["elf", 65536, 43, "x86", 0x3E, 64, True, [[4096, 30000, 1], [34096, 31000, 1]]],
                                           ["x86", 65536, 44], ["x86", 1000, 45]]]
STREAM_BLOCKS = 6
STREAM_CHAINS = [("EXE", "NONE", 0), ("EXE+RLT", "HUFFMAN", 0), ("EXE+ROLZX", "ANS0", 0), ("EXE+PACK+ZRLT", "FPAQ", 0),
                 ("EXE+BWT+RANK+ZRLT", "ANS0", 32)]
HOSTED = [("TEXT+EXE+RLT", "HUFFMAN", 65536, 0)]
CLI = ["concat", 300001, 0, [["x86", 200000, 50], ["text", 30001, 51], ["arm", 70000, 52]]]
CLI_ARGS = ["-t", "EXE+RLT", "-e", "HUFFMAN"]
# the timing input of tools/gpu_exe_time.py: blocks of 8 MiB of the x86 generator
TIME_UNIT = ["x86", 1 << 20, 60]
