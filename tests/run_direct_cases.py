"""Inputs for the run round's direct placement of the run members (k_bwt_f_run_emit, csrc/bwt_fwd.hip), shared by
tests/test_gpu_bwt_run_direct.py and tests/test_emu_bwt_run_direct.py, and a count of the run members made from the input alone.

The run round takes the suffixes that begin with nsym equal bytes c, per block and byte, when there are more than SM_G of them (a run
group). A run of length L >= nsym of such a byte has the members R = nsym .. L. The sorted members of one (byte, direction) -- direction:
the byte behind the run is smaller than c or the block ends there ("below"), or larger ("above") -- are the columns R of a ragged matrix
whose rows are the runs in the order of what follows them; the device cuts the rows into tiles of RUN_TILE and takes runs of up to
RUN_DIRECT_LMAX bytes."""
import re

import numpy as np

import knzlib
from unsplit_cases import SM_G, _rnd

RUN_TILE = 1024              # csrc/bwt_fwd.hip
RUN_DIRECT_LMAX = 1023       # csrc/bwt_fwd.hip
NSYM = 4                     # the synthetic inputs are sorted with this round-0 key length (knob bwt_nsym), so that the run counts below hold


def _runs(rng, byte, lengths, above, tails=True):
    """Runs of `byte` with the given lengths, each followed by one byte below it (or above it) and, with `tails`, three random bytes of
    that side as well (what follows decides the order of the runs)."""
    out = bytearray()
    for L in lengths:
        out += bytes([byte]) * int(L)
        lo, hi = (byte + 1, 256) if above else (0, byte)
        out += bytes(rng.integers(lo, hi, 4 if tails else 1, dtype=np.uint8).tolist())
    return bytes(out)


def both_directions(maxlen):
    """Runs of the lengths 1 .. maxlen (NSYM - 1, NSYM and NSYM + 1 among them) of a dozen bytes, each followed by a smaller byte or a
    larger one; the last run ends the block."""
    rng = np.random.default_rng(51)
    bytes_ = list(range(100, 112))
    out = bytearray()
    for i, L in enumerate(rng.permutation(np.arange(1, maxlen + 1)).tolist()):
        c = bytes_[i % 12]
        out += bytes([c]) * L
        out += bytes([int(rng.integers(0, 100)) if rng.integers(0, 2) else int(rng.integers(112, 256))])
    return bytes(out) + bytes([105]) * 37


def ties(reps):
    """Eight stretches (byte, length, eight bytes that follow), each `reps` times, random bytes between them: the members of the copies of
    a stretch tie on (R, what follows)."""
    rng = np.random.default_rng(52)
    st = []
    for s in range(8):
        c = 60 + 20 * (s % 4)
        tail = rng.integers(0, c, 8, dtype=np.uint8) if s < 4 else rng.integers(c + 1, 256, 8, dtype=np.uint8)
        st.append(bytes([c]) * int(rng.integers(5, 60)) + tail.tobytes())
    out = bytearray()
    for r in range(reps):
        for s in rng.permutation(8).tolist():
            out += st[s] + bytes(rng.integers(150, 256, 6, dtype=np.uint8).tolist())
    return bytes(out)


def multi_tile(extra, maxlen):
    """3 * RUN_TILE + extra runs of one byte, all followed by larger bytes, lengths NSYM .. maxlen (many equal): one segment of four
    tiles, the last nearly empty."""
    rng = np.random.default_rng(53)
    return _runs(rng, 128, rng.integers(NSYM, maxlen + 1, 3 * RUN_TILE + extra), True)


def tile_edge(maxlen):
    """Exactly RUN_TILE runs of one byte followed by smaller bytes (one full tile) and RUN_TILE + 1 of another followed by larger ones (a
    full tile and a tile of one run)."""
    rng = np.random.default_rng(54)
    a = _runs(rng, 90, rng.integers(NSYM, maxlen + 1, RUN_TILE), False)
    b = _runs(rng, 160, rng.integers(NSYM, maxlen + 1, RUN_TILE + 1), True)
    return a + b


def long_run(longest, n_other):
    """One run of `longest` bytes among shorter runs of the same byte, in both directions."""
    rng = np.random.default_rng(55)
    other = rng.integers(NSYM, 30, n_other)
    return _runs(rng, 77, other[:n_other // 2], True) + _runs(rng, 77, [longest], True) + _runs(rng, 77, other[n_other // 2:], False)


def batch(sizes):
    """Four blocks, the last shorter than NSYM; the same bytes have run groups in the first three (classes are per block). The emulator's
    driver takes blocks of any lengths; the device encoder cuts a buffer into blocks of one size, so there only the last one differs."""
    rng = np.random.default_rng(56)
    out = []
    for size in sizes:
        b = bytearray()
        while len(b) < size:
            b += _runs(rng, 40 + 30 * int(rng.integers(0, 3)), rng.integers(1, 50, 8), bool(rng.integers(0, 2)), tails=False)
        out.append(bytes(b[:size]))
    out.append(b"\x28\x28\x28")
    return out


def build(scale):
    """name -> (list of blocks, nsym forced to NSYM?, placed directly?) at full size (scale 1: the GPU test) or at what the emulator sorts
    in seconds (scale 0)."""
    big = scale == 1
    mixed = knzlib.corpus().mixed(5 << 18, 2)           # (segments 3 and 4 are the ones with runs: sparse pokes into zeros, runs of random bytes)
    out = {
        "both_directions": ([both_directions(600 if big else 140)], True, True),
        "ties": ([ties(400 if big else 60)], True, True),
        "multi_tile": ([multi_tile(5, 40 if big else 9)], True, True),
        "tile_edge": ([tile_edge(40 if big else 9)], True, True),
        "long_run_below_limit": ([long_run(RUN_DIRECT_LMAX, 3000 if big else 200)], True, True),
        "long_run_above_limit": ([long_run(RUN_DIRECT_LMAX + 1, 3000 if big else 200)], True, False),
        "one_byte_block": ([bytes([200]) * (65536 if big else 3000)], True, False),
        "batch": (batch((65536, 65536, 65536) if big else (6000, 3000, 2000)), True, True),
        "mixed": ([mixed[:1 << 20], mixed[1 << 20:]] if big else [mixed[(3 << 18):(3 << 18) + 20000] + mixed[(4 << 18):(4 << 18) + 20000]], False, True),
    }
    return out


def run_members(blocks, nsym):
    """Members of the run groups, counted from the input: per block and byte, the runs of at least nsym bytes contribute L - nsym + 1
    each; the byte has a run group when that is more than SM_G."""
    total = 0
    for b in blocks:
        a = np.frombuffer(b, dtype=np.uint8)
        if len(a) < nsym:
            continue
        cut = np.flatnonzero(a[1:] != a[:-1]) + 1
        starts = np.r_[0, cut]
        lens = np.diff(np.r_[starts, len(a)])
        keep = lens >= nsym
        per = np.bincount(a[starts[keep]], weights=(lens[keep] - nsym + 1), minlength=256)
        total += int(per[per > SM_G].sum())
    return total


_LINE = re.compile(r"after round 0 \(nsym (\d+), total \d+\): run groups (\d+) \((\d+) members\).*run members placed directly (\d+), sorted (\d+)")


def parse(err):
    """The "after round 0" lines the knob bwt_stats prints -> [(nsym, run groups, their members, placed directly, sorted)]"""
    return [tuple(int(x) for x in m.groups()) for m in _LINE.finditer(err)]
