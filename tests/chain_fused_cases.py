"""Inputs for the chain round run in place by k_bwt_f_medium_fused (csrc/bwt_fwd.hip: med_chain_round), shared by
tests/test_gpu_bwt_chain_fused.py and tests/test_emu_chain_fused.py.

A group takes the chain round when the majority of its members looks at the group itself: inside a stretch of period P, in the round
whose offset is P (or, for a period the probe found, in the first round, P positions on), a member's successor p + P is a member too,
but for the last member of every stretch: the chain's end, whose key is another label. The kernel sorts the ends by that key, then all
members on (chain length or its mirror, rank of the end's key). What can go wrong there depends on the number of ends (counted sort
up to the thread count, radix sort above, and the scratch arrays laid over the group's own LDS hold at most half the group's
capacity), on the chain lengths, on which side of the group's label the ends' keys lie, on ties, on the link and on the block bounds.

The CPU model is that of medium_fused_cases.class_sizes: classes of suffixes that agree in their first `depth` bytes. chain_groups()
lists, for the classes of medium size, how many members have their successor `link` bytes on in the class and how many are ends."""
import re

import numpy as np

import knzlib
import medium_fused_cases
from medium_fused_cases import MED_LO_CAP
from unsplit_cases import SM_G, MED_CAP, _rnd


def _unit(period, seed):
    """A random unit whose bytes are neither 0x00 nor 0xFF (a filler that begins with one of those lies below or above every unit byte)."""
    return np.random.default_rng(seed).integers(1, 255, period, dtype=np.uint8).tobytes()


def stretches(unit, copies, fillers):
    """One stretch `unit * m` per entry of `copies`, each followed by its filler."""
    return b"".join(unit * m + f for m, f in zip(copies, fillers))


def class_ids(data, k):
    """Class number of every suffix by its first k bytes (medium_fused_cases.class_sizes keeps the sizes only)."""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64) + 1
    n = len(a)
    key = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        c = np.zeros(n, dtype=np.uint64)
        c[:n - j] = a[j:]
        key = key * np.uint64(257) + c
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return inv.reshape(-1), cnt


def chain_groups(data, depth, link):
    """[(members, members whose successor `link` on is in the class, ends)] for the classes at `depth` of SM_G + 1 .. MED_CAP members in
    which at least half the members have their successor in the class: the groups the chain round takes."""
    inv, cnt = class_ids(data, depth)
    n = len(inv)
    linked = np.zeros(n, dtype=bool)
    linked[:n - link] = inv[:n - link] == inv[link:]
    per = np.bincount(inv, weights=linked, minlength=len(cnt)).astype(np.int64)
    return [(int(cnt[c]), int(per[c]), int(cnt[c] - per[c])) for c in np.flatnonzero((cnt > SM_G) & (cnt <= MED_CAP) & (2 * per >= cnt) & (per < cnt))]


def end_sides(data, depth, link):
    """(ends whose successor sorts below the class's own `depth` bytes, ends whose successor sorts above them) in the largest class that
    chain_groups() lists: what follows an end differs from what the members share, and the first byte that differs says on which side."""
    inv, cnt = class_ids(data, depth)
    n = len(inv)
    linked = np.zeros(n, dtype=bool)
    linked[:n - link] = inv[:n - link] == inv[link:]
    per = np.bincount(inv, weights=linked, minlength=len(cnt)).astype(np.int64)
    ok = np.flatnonzero((cnt > SM_G) & (cnt <= MED_CAP) & (2 * per >= cnt) & (per < cnt))
    c = ok[np.argmax(cnt[ok])]
    below = above = 0
    for e in np.flatnonzero((inv == c) & ~linked):
        own, nxt = data[e:e + depth], data[e + link:e + link + depth]
        if nxt < own:                                   # (bytes compare like suffixes: a proper prefix sorts first)
            below += 1
        else:
            above += 1
    return below, above


def build(scale):
    """name -> (blocks, nsym, period, (lo, hi], least number of ends): the batch, the round-0 key length the case needs (0: any), the
    depth and link at which chain_groups() must find a group of lo < members <= hi with at least that many ends. scale 1: blocks of one
    MiB (the GPU test); scale 0: periods and fillers reduced to what the emulator sorts in seconds."""
    P = 64 if scale == 1 else 16
    fl = 37 if scale == 1 else 11
    rng = np.random.default_rng(400)
    out = {}
    # more ends than threads: ~300 chains of 3-4 members (256 x 8), ~600 chains of 4-5 (512 x 16: the radix sort of the ends, and the most
    # ends the scratch arrays are asked to hold)
    u = _unit(P, 401)
    out["ends_above_threads_lower"] = ([stretches(u, rng.integers(4, 6, 300), [_rnd(fl, 410 + k) for k in range(300)])], 0, P, (SM_G, MED_LO_CAP), 257)
    u = _unit(P, 402)
    out["ends_above_threads_upper"] = ([stretches(u, rng.integers(5, 7, 600), [_rnd(fl, 1410 + k) for k in range(600)])], 0, P, (MED_LO_CAP, MED_CAP), 513)
    # one chain as long as the shape allows: 257, 2048, 2049 and 8192 copies
    blocks, _, nsym = medium_fused_cases.build(scale)["boundaries"]
    out["one_long_chain"] = (blocks, nsym, P, (MED_LO_CAP, MED_CAP), 1)
    # ends on both sides of the group's own label: the stretch is followed by 0x00 (below every unit byte) or by 0xFF (above)
    u = _unit(P, 403)
    out["ends_both_sides"] = ([stretches(u, rng.integers(4, 8, 150), [(b"\x00" if k & 1 else b"\xff") + _rnd(fl, 2410 + k) for k in range(150)])], 0, P, (SM_G, MED_LO_CAP), 150)
    # tied chains: pairs of stretches of equal length followed by the same 300 bytes (their members stay together and go on as children),
    # among chains that are not tied
    u = _unit(P, 404)
    copies = list(rng.integers(4, 8, 100)) + [m for m in rng.integers(4, 8, 40) for _ in (0, 1)]
    fillers = [_rnd(fl, 3410 + k) for k in range(100)] + [_rnd(300, 3600 + k) + bytes([j]) for k in range(40) for j in (1, 2)]
    out["tied_chains"] = ([stretches(u, copies, fillers)], 0, P, (SM_G, MED_LO_CAP), 180)
    # a link other than the round's offset: a period that is no power of two, found by k_bwt_f_probe before the first round; both shapes
    plo, phi = (700, 300) if scale == 1 else (70, 44)
    text = knzlib.corpus().text(2000, 5)
    out["probe_link_lower"] = ([text + _rnd(plo, 405) * 550], 0, plo, (SM_G, MED_LO_CAP), 1)
    out["probe_link_upper"] = ([text + _rnd(phi, 406) * 2500], 0, phi, (MED_LO_CAP, MED_CAP), 1)
    # block bounds: a group at a block's end, and two blocks in a batch
    for name in ("block_end", "two_blocks"):
        blocks, _, nsym = medium_fused_cases.build(scale)[name]
        out[name] = (blocks, nsym, P, (SM_G, MED_CAP), 1)
    return out


def check(name, blocks, period, size, ends):
    """Some block of the input holds a group the chain round takes, of the size class and with the number of ends the case is about."""
    found = [g for b in blocks for g in chain_groups(b, period, period)]
    assert any(size[0] < n <= size[1] and e >= ends for n, _, e in found), (name, sorted(found)[-5:])
    if name == "one_long_chain":
        assert {n for n, _, e in found if e == 1} >= {MED_LO_CAP - 1, MED_LO_CAP, MED_CAP - 1}, sorted(found)
    if name == "ends_both_sides":
        below, above = end_sides(blocks[0], period, period)
        assert below >= 50 and above >= 50, (below, above)


_CHAIN = re.compile(r"(\d+) groups took the chain round")


def chain_rounds(err):
    """The per-round lines the knob bwt_stats prints to stderr -> [groups that took the chain round]"""
    return [int(m.group(1)) for m in _CHAIN.finditer(err)]
