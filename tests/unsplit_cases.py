"""Inputs whose medium groups (257..8192 suffixes that agree so far) meet doubling rounds that cannot split them, shared by
tests/test_gpu_bwt_unsplit.py and tests/test_emu_bwt_unsplit.py, and a CPU model of the rounds that counts such groups.

A member of a group looks at the group h positions on. Inside a periodic stretch, a table or records with a shared prefix every member
finds the same group there; only the members within h of the stretch's end differ. A group in which all do agree comes out of the round as
it went in: k_bwt_f_gather_desc sees that and neither stores nor sorts it (knob bwt_no_unsplit_skip: off)."""
import re

import numpy as np

import knzlib

SM_G, MED_CAP = 256, 8192          # csrc/bwt_fwd.hip: a medium group has SM_G + 1 .. MED_CAP members


def _rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def ramp256(m, segs=6):
    """Byte ramps of period 256, `segs` stretches with ~m members per residue in all, random bytes between them: 256 groups that lose a
    member per stretch end and round until the offset is the period (chain round)."""
    per = 256 * (m // segs)
    return b"".join(bytes((np.arange(per + 37 * k) & 255).astype(np.uint8)) + _rnd(301, k) for k in range(segs))


def ramp768(m, stretches=2):
    """Period 768 (0 0 0 1 1 1 ... 255 255 255), m periods: no doubling offset is a multiple of the period, so a group never looks at
    itself and erodes from a stretch's end only -- unsplit in the round of offset h, split in the round of offset 2h. In TWO equal
    stretches the seam falls in the middle of every group, where k_bwt_f_probe_scan compares the distances of four neighbouring members:
    it finds no single period and leaves the groups to the doubling rounds. ONE stretch is what the probe takes apart before the first
    round (no medium group is left for the rounds: the streams are compared all the same)."""
    one = bytes((np.arange(768 * (m // stretches)) % 768 // 3).astype(np.uint8))
    return b"".join(one + _rnd(301 + 199 * k, 7 + k) for k in range(stretches))


def records(r):
    """r records of 300 bytes that share their first 200: a group per prefix offset, unsplit until the offset reaches the random tail."""
    head = _rnd(200, 11)
    tails = np.random.default_rng(12).integers(0, 256, (r, 100), dtype=np.uint8)
    return b"".join(head + tails[i].tobytes() for i in range(r))


def stretches(m1, m2, period=64):
    """Two periodic stretches of random units, m1 and m2 members per residue (at full size 6,000: a medium group of more than half of
    MED_CAP, and 9,000: above MED_CAP, large groups that shed medium ones), text between them."""
    return _rnd(period, 21) * m1 + knzlib.corpus().text(20000, 9) + _rnd(period, 22) * m2


def build(scale):
    """name -> (bytes, periodic?) at full size (scale 1: the GPU test, blocks of 1 MiB) or reduced to what the emulator sorts in seconds."""
    if scale == 1:
        m, m768, r, m1, m2, nt = 3072, 1000, 3000, 6000, 9000, 600000
    else:
        m, m768, r, m1, m2, nt = 288, 260, 270, 300, 420, 30000
    return {
        "ramp256": (ramp256(m), True),
        "ramp768": (ramp768(m768), True),
        "ramp768_one_stretch": (ramp768(m768, 1), False),
        "records": (records(r), True),
        "stretches": (stretches(m1, m2, 64 if scale == 1 else 16), True),
        "text": (knzlib.corpus().text(nt, 4), False),
    }


def unsplit_rounds_model(data, h0=4, rounds=6, cap=MED_CAP):
    """Prefix doubling on the CPU: classes of suffixes equal in their first h bytes (end of block sorts first), h = h0, 2 h0, ...
    Returns per round the number of classes of SM_G + 1 .. cap members that are still ONE class at 2h (no member differs h on), and the
    largest number of consecutive rounds one and the same class stayed so."""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.int64) + 1
    n = len(a)
    rank = np.zeros(n, dtype=np.int64)

    def dense(keys):                       # lexicographic rank of the key tuples (last key is the primary one for np.lexsort)
        order = np.lexsort(keys)
        ks = [k[order] for k in keys]
        new = np.ones(n, dtype=bool)
        new[1:] = np.any([k[1:] != k[:-1] for k in ks], axis=0)
        r = np.empty(n, dtype=np.int64)
        r[order] = np.cumsum(new) - 1
        return r

    cols = []
    for k in range(h0):                    # classes on the first h0 bytes
        c = np.zeros(n, dtype=np.int64)
        c[:n - k] = a[k:]
        cols.append(c)
    rank = dense(cols[::-1])
    counts, streak, best = [], {}, 0
    h = h0
    for _ in range(rounds):
        nxt = np.zeros(n, dtype=np.int64)
        nxt[:n - h] = rank[h:] + 1
        rank2 = dense([nxt, rank])
        size = np.bincount(rank)
        order = np.argsort(rank, kind="stable")
        r_sorted, r2_sorted = rank[order], rank2[order]
        start = np.r_[True, r_sorted[1:] != r_sorted[:-1]]
        lo = np.minimum.reduceat(r2_sorted, np.flatnonzero(start))
        hi = np.maximum.reduceat(r2_sorted, np.flatnonzero(start))
        split = lo != hi
        medium = (size > SM_G) & (size <= cap) & ~split
        counts.append(int(medium.sum()))
        # a class is named by its smallest member: the name survives a round that does not split it
        names = np.minimum.reduceat(order, np.flatnonzero(start))
        cur = {}
        for nm in names[medium]:
            cur[int(nm)] = streak.get(int(nm), 0) + 1
            best = max(best, cur[int(nm)])
        streak = cur
        rank = rank2
        h *= 2
    return counts, best


_STAT = re.compile(r"medium groups worked on (\d+) \((\d+) members\): all keys equal in (\d+) \((\d+) members\)( -- left alone)?")


def parse_stats(err):
    """The per-round lines the knob bwt_stats prints to stderr -> [(groups, members, unsplit groups, unsplit members, skipped?)]"""
    return [(int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5) is not None) for m in _STAT.finditer(err)]
