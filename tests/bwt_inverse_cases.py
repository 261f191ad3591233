"""Inputs for the inverse BWT's paths (csrc/bwt.hip), shared by tests/test_gpu_bwt_inverse.py, the emulator run in
tests/test_emu_kernels.py, tests/test_oracle_vs_ref.py and the generator tests/golden/make_first_gen_damage.py.

Sizes: sub-lists of the splitter walk have 64 nodes on average and a row of symbols (ROW) holds 128 (63 .. 129), bwt_chunks goes from
one primary index to eight at 256, one tile of the counting sort (IT) is 4096 bytes, bwt_i_seg_tiles changes the segment size between 4
and 5 and between 16 and 17 tiles, and 300,001 is a block of many tiles with a ragged tail. INV_NARROW_MAX = 2^23 is the longest block whose link records are 4-byte words."""
import numpy as np

import knzlib

SIZES = (2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 4095, 4096, 4097, 4 * 4096, 4 * 4096 + 1, 16 * 4096, 16 * 4096 + 1, 300001)
CONTENTS = ("text", "twosym", "const", "ab", "ramp")
INV_NARROW_MAX = 1 << 23                 # csrc/bwt.hip

RAGGED_BS = 16384
RAGGED_CHAINS = (("RLT+BWT", "NONE"), ("RLT+BWT+MTFT+ZRLT", "ANS0"))
RAGGED_STAGE_LENGTHS = [10, 16375, 358, 16384, 16277, 10, 16384, 1]

HEADER_SPECS = (("text", 300, 3), ("text", 5000, 3))


def block(kind, n):
    c = knzlib.corpus()
    if kind == "text":
        return c.text(n, 3)
    if kind == "twosym":
        return bytes((np.random.default_rng(n).integers(0, 2, n) * 7 + 60).astype(np.uint8))
    if kind == "const":                  # every sub-list of the walk overruns its row: the rows come from InvInfo::dyn
        return bytes([7]) * n
    if kind == "ab":
        return (b"ab" * (n // 2 + 1))[:n]
    if kind == "ramp":
        return (bytes(range(256)) * (n // 256 + 1))[:n]
    raise ValueError(kind)


def single_blocks():
    """[(name, bytes)] for every size and content."""
    return [("%s_%d" % (kind, n), block(kind, n)) for n in SIZES for kind in CONTENTS]


def ragged_data():
    """Eight blocks of RAGGED_BS bytes (the last: one byte) behind whose RLT stage the BWT stage sees the lengths RAGGED_STAGE_LENGTHS
    in one batch (16,384: RLT refuses the block)."""
    import vectors
    c = knzlib.corpus()
    bs = RAGGED_BS
    blocks = [
        bytes(bs),
        c.text(bs, 5),
        (vectors.make(("runs", 300, 400)) * 2)[:bs],
        b"ab" * (bs // 2),
        (bytes([7]) * 100 + c.text(bs, 6))[:bs],
        bytes([1]) * bs,
        c.mixed(300000, 2)[250000:250000 + bs],
        b"x",
    ]
    assert all(len(b) == bs for b in blocks[:-1])
    return blocks


def ragged_stage_lengths(oracle):
    """What the oracle's RLT leaves of every block (the block itself where it refuses)."""
    out = []
    for b in ragged_data():
        ok, o = oracle.forward("RLT", b, len(b))
        out.append(len(o) if ok else len(b))
    return out


def header_len(enc):
    """Bytes of the block header of bitstream version 6 (BWTBlockCodec.cpp:106-118): a mode byte, then 2^k indexes of 1..4 bytes."""
    mode = enc[0]
    return 1 + (1 << ((mode >> 2) & 7)) * ((mode & 3) + 1)


def header_damage(enc, n):
    """The damaged forms of one encoded block `enc` of an n-byte input: [(damage as (offset, value) pairs, length the block is cut to,
    destination capacity)]. The capacity is the encoded length (the reference's sequence wants a destination no shorter than its input)
    but for the last case."""
    h = header_len(enc)
    cap = len(enc)
    out = []
    for off in range(h):
        b = enc[off]
        for v in (0, 0xFF, b ^ 1, b ^ 4, b ^ 0x80, (b + 1) & 0xFF):
            out.append((((off, v),), len(enc), cap))
    out.append(((), h, cap))                      # the header alone
    out.append(((), h + 1, cap))                  # ... and one byte
    out.append(((), len(enc) - 1, cap))           # the last byte dropped
    out.append(((), len(enc), n - 1))             # a destination one byte short
    return out


def apply(enc, damage, cut):
    b = bytearray(enc)
    for off, v in damage:
        b[off] = v
    return bytes(b[:cut])
