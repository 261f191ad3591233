"""Inputs for the run round's placement from the run tables alone (k_bwt_f_run_tie_marks, k_bwt_f_run_emit, k_bwt_f_run_place<true>) and
for round 0's gaps that are filled at their ends only (R0_GAP_MARGIN; k_bwt_f_r0_fill, _flags, _place_text), csrc/bwt_fwd.hip. Shared by
tests/test_gpu_bwt_run_tables.py and tests/test_emu_bwt_run_tables.py.

Two members of a column (byte, direction, R) tie when the text behind their runs has the same label, which round 0 gives by the first
NSYM bytes (and, in a group of up to SM_G suffixes, by seven more): runs of one (byte, direction) followed by the same TAIL_SAME bytes
are a STRETCH of equal sort keys, adjacent among the sorted runs. Which members of a stretch start a tie is decided from the lengths of
the runs in front of them; the cases put stretches where that decision crosses the units of the kernels (rows of 64 runs, tiles of
RUN_TILE runs, the first and the last runs of a segment, placement workgroups of 256 members that span classes)."""
import re

import numpy as np

import run_direct_cases
from run_direct_cases import NSYM, RUN_TILE
from unsplit_cases import SM_G

R0_GAP_MARGIN = 2048         # csrc/bwt_fwd.hip
TAIL_SAME = 12               # bytes the runs of a stretch share behind them: NSYM + 7 and one more


def _tail(first, ident):
    """TAIL_SAME bytes that begin with `first`, the same for the same `ident` and different in the first NSYM bytes for different ones
    (no byte of a run group among them: 1 .. 47 behind the first)."""
    r = np.random.default_rng([77, ident])
    body = r.integers(1, 48, TAIL_SAME - 1, dtype=np.uint8).tolist()
    body[0], body[1], body[2] = 1 + ident % 47, 1 + (ident // 47) % 47, 1 + (ident // (47 * 47)) % 47
    return bytes([first] + body)


def _unique(i):
    """four bytes that differ from run to run (what follows a stretch's shared bytes)"""
    return bytes([48 + (i & 15), 48 + ((i >> 4) & 15), 48 + ((i >> 8) & 15), 48 + ((i >> 12) & 15)])


def _emit(byte, runs, order_seed):
    """runs = [(length, tail bytes)]: the runs of `byte` in a shuffled text order, each with its tail and four unique bytes behind it"""
    rng = np.random.default_rng(order_seed)
    out = bytearray()
    for i in rng.permutation(len(runs)).tolist():
        L, tail = runs[i]
        out += bytes([byte]) * int(L) + tail + _unique(i)
    return bytes(out)


def heads_inside_a_stretch(reps):
    """One byte, one direction, every run followed by the same bytes: one stretch. In text order the lengths repeat 5, 9, 7, 9, 30, 4, 30,
    12; the sorted order of the runs of a stretch is their text order, so the first 9 and the first 30 start the ties of the columns
    above 5 and above 9, and no later run starts one."""
    c = 120
    tail = _tail(3, 0)
    out = bytearray()
    for i in range(reps):
        for L in (5, 9, 7, 9, 30, 4, 30, 12):
            out += bytes([c]) * L + tail + _unique(len(out) & 0xFFFF)
    return bytes(out)


def stretch_across_rows(maxlen):
    """A segment (byte 100, followed by larger bytes) of 300 runs: 50 with tails of their own that sort in front, a stretch of 200 that
    begins at run 50 and crosses three rows of 64, 50 with tails of their own behind it. Lengths NSYM .. maxlen."""
    rng = np.random.default_rng(61)
    L = rng.integers(NSYM, maxlen + 1, 300).tolist()
    runs = [(L[i], _tail(110 + i % 40, 1 + i)) for i in range(50)]
    runs += [(L[50 + i], _tail(150, 0)) for i in range(200)]
    runs += [(L[250 + i], _tail(160 + i % 40, 100 + i)) for i in range(50)]
    return _emit(100, runs, 62)


def stretch_across_tiles(maxlen):
    """A segment of about 2200 runs, three tiles: stretches of one to three runs, then one stretch from run 1000 to run 2100, then
    stretches of one to three runs again."""
    rng = np.random.default_rng(63)
    runs, ident = [], 1
    while len(runs) < 1000:
        k = min(int(rng.integers(1, 4)), 1000 - len(runs))
        runs += [(int(rng.integers(NSYM, maxlen + 1)), _tail(130 + ident % 30, ident)) for _ in range(k)]
        ident += 1
    runs += [(int(rng.integers(NSYM, maxlen + 1)), _tail(170, 0)) for _ in range(1100)]
    while len(runs) < 2200:
        k = min(int(rng.integers(1, 4)), 2200 - len(runs))
        runs += [(int(rng.integers(NSYM, maxlen + 1)), _tail(180 + ident % 30, ident)) for _ in range(k)]
        ident += 1
    assert 1000 < RUN_TILE and 2 * RUN_TILE < 2100 < len(runs) <= 3 * RUN_TILE         # (the stretch crosses both tile boundaries)
    return _emit(125, runs, 64)


def stretch_first_and_last(maxlen):
    """Both directions of byte 140, a stretch of 70 runs at either end of both segments and runs with tails of their own between them;
    the block ends in a run (T = 0: the first run of the segment of the smaller followers, in front of its first stretch)."""
    rng = np.random.default_rng(65)

    def seg(lo_first, mid_first, hi_first, ident0):
        r = [(int(rng.integers(NSYM, maxlen + 1)), _tail(lo_first, ident0)) for _ in range(70)]
        r += [(int(rng.integers(NSYM, maxlen + 1)), _tail(mid_first + i % 20, ident0 + 1 + i)) for i in range(40)]
        r += [(int(rng.integers(NSYM, maxlen + 1)), _tail(hi_first, ident0 + 50)) for _ in range(70)]
        return r
    runs = seg(60, 70, 139, 0) + seg(141, 150, 255, 100)
    return _emit(140, runs, 66) + bytes([140]) * 23


def classes_inside_a_workgroup():
    """Three blocks of 16 KiB with 40 bytes each that have just over SM_G members: a placement workgroup of 256 members spans two or three
    classes, and the class tables are per block."""
    rng = np.random.default_rng(67)
    blocks = []
    for b in range(3):
        out = bytearray()
        for c in range(50, 90):
            members = SM_G + 1 + int(rng.integers(0, 12))
            lens = [40] * 6 + [members - 6 * 37 + NSYM - 1]
            out += run_direct_cases._runs(rng, c, lens, bool(rng.integers(0, 2)))
        assert len(out) <= 16384
        out += bytes(rng.integers(128, 256, 16384 - len(out), dtype=np.uint8).tolist())        # (noise: no run group)
        blocks.append(bytes(out))
    return blocks


def big_gap():
    """Two blocks (a workgroup of the flag kernel spans both: the block size is no multiple of its 2048 slots). In each: a gap of zeros
    of 20,013 members that starts 3 slots behind the block's first (the block ends in three zeros, short suffixes, which sort in front),
    gaps of exactly 2 * R0_GAP_MARGIN members and of one more (bytes 7 and 9), and a gap of byte 255, 6,000 members, which ends the
    block's slots."""
    rng = np.random.default_rng(68)
    blocks = []
    for b in range(2):
        runs = [(0, 503)] * 39 + [(0, 516)]                                            # members: L - NSYM + 1 each
        runs += [(7, 515)] * 8 + [(9, 515)] * 7 + [(9, 516)] + [(255, 503)] * 12
        out = bytearray()
        for i in rng.permutation(len(runs)).tolist():
            c, L = runs[i]
            out += bytes([c]) * L + bytes(rng.integers(16, 250, 4, dtype=np.uint8).tolist())
        size = 45008                                                                    # a multiple of 16, not of 256
        assert len(out) + 3 <= size and size % 16 == 0 and size % 256 != 0
        out += bytes(rng.integers(16, 250, size - 3 - len(out), dtype=np.uint8).tolist()) + bytes(3)
        blocks.append(bytes(out))
    per = {c: sum(L - NSYM + 1 for cc, L in runs if cc == c) for c in (0, 7, 9, 255)}
    assert per == {0: 20013, 7: 2 * R0_GAP_MARGIN, 9: 2 * R0_GAP_MARGIN + 1, 255: 6000}
    assert all(x % d for x in (3, 3 + per[0]) for d in (256, 1792, 2048))
    return blocks


def build(scale):
    """name -> (list of blocks, nsym forced to NSYM?, placed directly?, flag workgroups inside a gap: True some / False none / None not
    asserted), at full size (scale 1: the GPU test) or at what the emulator sorts in seconds (scale 0)"""
    big = scale == 1
    out = {
        "heads_inside_a_stretch": ([heads_inside_a_stretch(400 if big else 60)], True, True, None),
        "stretch_across_rows": ([stretch_across_rows(40)], True, True, None),
        "stretch_across_tiles": ([stretch_across_tiles(40 if big else 9)], True, True, None),
        "stretch_first_and_last": ([stretch_first_and_last(40)], True, True, None),
        "classes_inside_a_workgroup": (classes_inside_a_workgroup(), True, True, False),
        "big_gap": (big_gap(), True, True, True),
    }
    for name, (blocks, forced, direct) in run_direct_cases.build(scale).items():
        out["direct_" + name] = (blocks, forced, direct, None)
    return out


_SKIP = re.compile(r"after round 0 \(.*flag workgroups inside a gap (\d+)")


def parse_skipped(err):
    """The "after round 0" lines the knob bwt_stats prints -> [workgroups of k_bwt_f_r0_flags that lay inside a gap]"""
    return [int(m.group(1)) for m in _SKIP.finditer(err)]
