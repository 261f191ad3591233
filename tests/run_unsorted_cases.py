"""Inputs for round 0 without the run members (FwdSort::run_scan, TextSrcKept, LastPassSrc, k_bwt_f_r0_fill in csrc/bwt_fwd.hip), shared by
tests/test_gpu_bwt_run_unsorted.py and tests/test_emu_bwt_run_unsorted.py.

A suffix that starts with nsym copies of a byte c, full length, is a run member when its block holds more than SM_G of them (a run group,
or class). Such members stay out of round 0's sort: the first pass drops them, the last pass leaves a gap of their size in the slots of c,
the gap is filled with one key, and the run round writes every member. Each input below is chosen for one way that can go wrong; how many
members there are is counted from the input alone (run_direct_cases.run_members), per class by class_members below."""
import re

import numpy as np

import knzlib
import run_direct_cases
from run_direct_cases import RUN_DIRECT_LMAX
from unsplit_cases import SM_G

RS_TILE = 8192               # csrc/prims.hpp: elements of a tile of the radix passes


def _noise(n, seed, lo=100, hi=256):
    """Random bytes of [lo, hi): the run bytes of the cases are below lo, so noise adds no member to their classes."""
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def class_members(block, nsym):
    """byte -> full-length suffixes of the block that start with nsym copies of it"""
    a = np.frombuffer(block, dtype=np.uint8)
    if len(a) < nsym:
        return {}
    cut = np.flatnonzero(a[1:] != a[:-1]) + 1
    starts = np.r_[0, cut]
    lens = np.diff(np.r_[starts, len(a)])
    keep = lens >= nsym
    per = np.bincount(a[starts[keep]], weights=(lens[keep] - nsym + 1), minlength=256)
    return {c: int(per[c]) for c in np.flatnonzero(per)}


def _spread(byte, members, nsym, pieces, rng, sep_lo=100):
    """Runs of `byte` with `members` members in all, in `pieces` runs, noise between them."""
    cuts = np.sort(rng.choice(np.arange(1, members), pieces - 1, replace=False)) if pieces > 1 else np.array([], dtype=np.int64)
    parts = np.diff(np.r_[0, cuts, members])
    out = bytearray()
    for m in parts.tolist():
        out += bytes([byte]) * (m + nsym - 1) + _noise(int(rng.integers(1, 9)), int(rng.integers(1 << 30)), sep_lo)
    return bytes(out)


def sm_g_edge(nsym=4):
    """Byte 50 has exactly SM_G members (no run group: it stays in the sort), byte 60 has SM_G + 1 (the smallest gap)."""
    rng = np.random.default_rng(61)
    b = _noise(700, 1) + _spread(50, SM_G, nsym, 5, rng) + _noise(300, 2) + _spread(60, SM_G + 1, nsym, 4, rng) + _noise(500, 3)
    cm = class_members(b, nsym)
    assert cm.get(50) == SM_G and cm.get(60) == SM_G + 1
    return b


def two_bytes(n):
    """Only gaps and short suffixes, nearly: n sevens, then n nines. The run of 7 is followed by a run of another class (the label of the
    position behind it is a gap's first slot), the run of 9 by the block end."""
    return bytes([7]) * n + bytes([9]) * n


def end_run(byte, n, run):
    """A block that ends in a run: its last nsym - 1 suffixes are short; those of zeros pad to the class's own key and sit right in
    front of the gap, those of another byte are smaller keys."""
    rng = np.random.default_rng(62 + byte)
    return _noise(n // 2, 4) + _spread(byte, 400, 4, 6, rng) + _noise(n // 2, 5) + bytes([byte]) * run


def behind_runs(kind, reps):
    """Runs of 30 and of 80 (both classes) whose successor is, by `kind`: a run of the other class (from below and from above), a run of a
    byte without a run group (70: a few short runs), or the block end (the block's last run)."""
    rng = np.random.default_rng(63)
    out = bytearray()
    for r in range(reps):
        la, lb = int(rng.integers(4, 40)), int(rng.integers(4, 40))
        if kind == "class":
            out += bytes([30]) * la + bytes([80]) * lb + _noise(3, r) + bytes([80]) * lb + bytes([30]) * la + _noise(2, r + 1000)
        elif kind == "no_class":
            out += bytes([30]) * la + (bytes([70]) * int(rng.integers(4, 7)) if r < 12 else bytes([70])) + bytes([80]) * lb + bytes([71]) + _noise(3, r)
        else:
            out += bytes([30]) * la + _noise(2, r) + bytes([80]) * lb + _noise(2, r + 1000)
    if kind == "end":
        out += bytes([30]) * 23
    b = bytes(out)
    cm = class_members(b, 4)
    assert cm[30] > SM_G and cm[80] > SM_G and cm.get(70, 0) <= SM_G
    return b


def tile_of_members(poke):
    """Zeros over more than two tiles of the first pass, noise behind them. Element i of the pass is position i - (nsym - 1) (the short
    suffixes come first), so with nsym = 4 the second tile holds the positions RS_TILE - 3 .. 2 RS_TILE - 4: members all of them -- the
    tile ranks nothing -- or, with a byte poked into position RS_TILE - 3, all but the tile's first element (the three positions in front
    of the poke, whose keys hold it too, belong to the first tile)."""
    b = bytearray(2 * RS_TILE + 3000)
    if poke:
        b[RS_TILE - 3] = 5
    return bytes(b) + _noise(3000, 6)


def _fit(b, size, seed):
    return (b + _noise(size, seed))[:size]


def batch(size):
    """Blocks of one size with different classes: zeros with pokes; runs of 40 and 70; noise alone (no class at all); runs of 40 and a tail
    of zeros; and a last block shorter than the key."""
    rng = np.random.default_rng(64)
    z = bytearray(size)
    for p in rng.integers(0, size, size // 64):
        z[p] = int(rng.integers(1, 256))
    r1 = b"".join(_spread(c, 300 + 40 * k, 4, 7, rng) for k, c in enumerate((40, 70, 40)))
    r2 = _spread(40, 500, 4, 9, rng)
    return [bytes(z), _fit(r1, size, 7), _noise(size, 8), _fit(r2, size - 64, 9) + bytes(64), b"\x28\x28\x28"]


def build(scale):
    """name -> (list of blocks, round-0 key length forced with the knob bwt_nsym or 0) at GPU size (scale 1: up to 256 KiB per block, all
    blocks of a case but the last of one size, a multiple of 16) or at what the emulator sorts in seconds (scale 0)."""
    big = scale == 1
    mixed = knzlib.corpus().mixed(5 << 18, 2)
    kinds = [mixed[k << 18:(k + 1) << 18] if big else mixed[k << 18:(k << 18) + 6000] for k in range(5)]
    out = {
        "sm_g_edge": ([sm_g_edge()], 4),
        "one_byte_block": ([bytes([200]) * (65536 if big else 3000)], 4),
        "two_bytes": ([two_bytes(30000 if big else 1500)], 4),
        "two_bytes_nsym5": ([two_bytes(30000 if big else 1500)], 5),
        "end_zero_run": ([end_run(0, 60000 if big else 4000, 700)], 4),
        "end_byte_run": ([end_run(33, 60000 if big else 4000, 700)], 4),
        "behind_class": ([behind_runs("class", 600 if big else 60)], 4),
        "behind_class_nsym5": ([behind_runs("class", 600 if big else 60)], 5),
        "behind_no_class": ([behind_runs("no_class", 600 if big else 60)], 4),
        "behind_end": ([behind_runs("end", 600 if big else 60)], 4),
        "tile_all_members": ([tile_of_members(False)], 4),
        "tile_one_other": ([tile_of_members(True)], 4),
        "member_sort": ([run_direct_cases.long_run(RUN_DIRECT_LMAX + 1, 3000 if big else 200)], 4),
        "batch": (batch(65536 if big else 4096), 4),
        "batch_nsym5": (batch(65536 if big else 4096), 5),
        # (the key length forced here too: the encoder sorts a buffer in batches that choose their own, and the count below needs to know it)
        "mixed_kinds": (kinds, 4),
        "mixed_kinds_nsym5": (kinds, 5),
    }
    return out


def run_members(blocks, nsym):
    return run_direct_cases.run_members(blocks, nsym)


_LINE = re.compile(r"after round 0 \(nsym (\d+), total \d+\): run groups (\d+) \((\d+) members\).*kept out of the round-0 sort (\d+)")


def parse(err):
    """The "after round 0" lines the knob bwt_stats prints -> [(nsym, run groups, their members, members kept out of the sort)]"""
    return [tuple(int(x) for x in m.groups()) for m in _LINE.finditer(err)]
