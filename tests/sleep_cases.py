"""Inputs whose medium groups can sleep through doubling rounds (k_bwt_f_med_sleep, csrc/bwt_fwd.hip), shared by tests/test_gpu_bwt_sleep.py
and tests/test_emu_bwt_sleep.py, and a CPU model of the rounds that applies the sleeping rule to the true classes.

The rule: G slept through the round of offset 2h when, in the round of offset h, all members of G found one group G' h positions on, all
members of G' found one group G'', and G'' came out of that round whole -- then every member of G finds G'' 2h positions on, and nobody
has to read a member to know it. Groups whose offset is not the plain h (a run tie: the members begin with a run of four equal symbols)
never sleep and nobody sleeps on their verdict, though they may be the G'' that stays whole."""
import re

import numpy as np

import knzlib
import unsplit_cases
from unsplit_cases import SM_G, MED_CAP, _rnd


def run_ties(r, run=48, shared=120):
    """r records of [`run` zero bytes][`shared` bytes all records share][40 random bytes]: the suffixes that begin inside the zeros are run
    groups; the run round leaves the r members with the same run length tied (the shared bytes follow), a medium group that looks
    max(run length, h) positions on -- an override, so it must be gathered in every round -- and stays whole until the tails are in sight."""
    head = bytes(run) + _rnd(shared, 31)
    tails = np.random.default_rng(32).integers(0, 256, (r, 40), dtype=np.uint8)
    return b"".join(head + tails[i].tobytes() for i in range(r))


def target_splits(r, r2):
    """r records of 300 bytes that share their first 200 (H), and r2 short records H[100:160] + random bytes. The group of prefix offset j
    in 100..159 holds r + r2 members until the short records' random bytes are in sight: it splits while the groups in front of it, which
    look at it (members of the full records only), are still whole on one key -- their target changed, so they must be gathered that round."""
    head = _rnd(200, 41)
    tails = np.random.default_rng(42).integers(0, 256, (r, 100), dtype=np.uint8)
    shorts = np.random.default_rng(43).integers(0, 256, (r2, 40), dtype=np.uint8)
    return b"".join(head + tails[i].tobytes() for i in range(r)) + b"".join(head[100:160] + shorts[i].tobytes() for i in range(r2))


def build(scale):
    """name -> bytes at full size (scale 1: the GPU test, one block of 1 MiB) or reduced to what the emulator sorts in seconds."""
    u = unsplit_cases.build(scale)
    r, r2 = (2600, 2600) if scale == 1 else (270, 270)      # (scale 1: 1,040,000 bytes, groups of 5,200)
    out = {k: u[k][0] for k in ("ramp256", "ramp768", "records", "stretches", "text")}
    out["run_ties"] = run_ties(r)
    out["target_splits"] = target_splits(r, r2)
    return out


def sleep_rounds_model(data, h0=4, rounds=7, cap=MED_CAP):
    """Prefix doubling on the CPU (classes of suffixes equal in their first h bytes, h = h0, 2 h0, ...; the end of the block sorts first),
    with the sleeping rule evaluated on the true classes. Returns [(offset, classes asleep, members asleep)] per round; the first round
    has no round before it and is always (h0, 0, 0)."""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.int64) + 1
    n = len(a)

    def dense(keys):                       # lexicographic rank of the key tuples (last key is the primary one for np.lexsort)
        order = np.lexsort(keys)
        ks = [k[order] for k in keys]
        new = np.ones(n, dtype=bool)
        new[1:] = np.any([k[1:] != k[:-1] for k in ks], axis=0)
        r = np.empty(n, dtype=np.int64)
        r[order] = np.cumsum(new) - 1
        return r

    cols = []
    for k in range(h0):
        c = np.zeros(n, dtype=np.int64)
        c[:n - k] = a[k:]
        cols.append(c)
    rank = dense(cols[::-1])
    # a run tie: the suffix begins with four equal symbols inside the block (what round 0 hands to the run round)
    runpos = np.zeros(n, dtype=bool)
    runpos[:n - 3] = (a[:n - 3] == a[1:n - 2]) & (a[:n - 3] == a[2:n - 1]) & (a[:n - 3] == a[3:])
    out, h = [], h0
    plain = whole = tgt = prev_rank = None
    for _ in range(rounds):
        nxt = np.zeros(n, dtype=np.int64)
        nxt[:n - h] = rank[h:] + 1
        size = np.bincount(rank)
        order = np.argsort(rank, kind="stable")
        first = np.flatnonzero(np.r_[True, rank[order][1:] != rank[order][:-1]])
        lo = np.minimum.reduceat(nxt[order], first)
        hi = np.maximum.reduceat(nxt[order], first)
        medium = (size > SM_G) & (size <= cap)
        override = runpos[order][first]                       # (of a class: all members begin alike)
        if plain is None:
            out.append((h, 0, 0))
        else:
            # the classes of the round before (prev_rank) that the rule puts to sleep in this round
            t1 = np.where(plain, tgt, 0)
            ok1 = plain & plain[t1]
            t2 = np.where(ok1, tgt[t1], 0)
            cls = np.arange(len(plain))
            asleep = ok1 & whole[t2] & (t1 != cls) & (t2 != cls)
            out.append((h, int(asleep.sum()), int(np.bincount(prev_rank)[asleep].sum())))
        whole = medium & (lo == hi)
        plain = whole & (lo > 0) & ~override
        tgt = np.maximum(lo - 1, 0)
        prev_rank = rank
        rank = dense([nxt, rank])
        h *= 2
    return out


_SLEEP = re.compile(r"asleep (\d+) \((\d+) members\)")


def parse_sleep(err):
    """The per-round lines the knob bwt_stats prints to stderr -> [(groups asleep, members asleep)]"""
    return [(int(m.group(1)), int(m.group(2))) for m in _SLEEP.finditer(err)]


_ROUND = re.compile(r"round h=(\d+) \([0-9.]+ ms\): (.*)")


def parse_rounds(err):
    """The rounds' own lines without their times: offsets, members worked on, groups left"""
    return [(int(m.group(1)), m.group(2)) for m in _ROUND.finditer(err)]
