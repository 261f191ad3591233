"""Inputs for k_bwt_f_medium_fused (csrc/bwt_fwd.hip), which fetches, judges and sorts a medium group (257..8192 suffixes that agree so
far) in one workgroup, shared by tests/test_gpu_bwt_medium_fused.py and tests/test_emu_medium_fused.py: the cases of
tests/unsplit_cases.py, and the smallest shapes at which the two size classes (up to 2048 members: 256 threads x 8; above: 512 x 16),
the per-class index, the block bounds and the past-the-end key can go wrong.

A stretch `unit * m` of a random unit of P bytes holds, per residue, the m suffixes that begin there: after round 0 (four or five
symbols) a group of exactly m members for the residues whose first symbols lie inside the unit in the last copy too, m - 1 for the few
others. Its members all look at the group of the residue h further on, but the last copy's: unsplit or majority path until h reaches
P, then the chain round."""
import re

import numpy as np

import knzlib
import unsplit_cases
from unsplit_cases import SM_G, MED_CAP, _rnd

MED_LO_CAP = 2048                  # csrc/bwt_fwd.hip: the larger groups go to the 512 x 16 workgroups


def sized(sizes, period, seed):
    """One stretch per size (a random unit of `period` bytes, m copies), random bytes between them."""
    return b"".join(_rnd(period, seed + k) * m + _rnd(401, 1000 + seed + k) for k, m in enumerate(sizes))


def marked(n, seed):
    """n records of seven shared bytes and two random ones: a group whose members all look at different groups (the plain radix sort)."""
    tails = np.random.default_rng(seed).integers(0, 256, (n, 2), dtype=np.uint8)
    return b"".join(b"abcdefg" + tails[i].tobytes() for i in range(n))


def class_sizes(data, k):
    """Sizes of the classes of suffixes that agree in their first k bytes (a suffix shorter than k stands alone: the end sorts first),
    by position: what round 0 makes with a key of k symbols."""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64) + 1
    n = len(a)
    key = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        c = np.zeros(n, dtype=np.uint64)
        c[:n - j] = a[j:]
        key = key * np.uint64(257) + c
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return cnt[inv]


def round0_sizes(data):
    """The group sizes round 0 makes of a block with a key of four and of five symbols (it chooses by the data's entropy)."""
    return [set(np.unique(class_sizes(data, k)).tolist()) for k in (4, 5)]


def build(scale):
    """name -> (blocks, group sizes the blocks must hold, nsym): the cases of this file. blocks: the byte strings of a batch, in order (all
    but the last one as long as the block size used: scale 1 is one MiB, the GPU test; scale 0 is what the emulator sorts in seconds and
    its harness takes block by block). nsym: 4 where the case needs round 0's key to be four symbols (the knob bwt_nsym), else 0."""
    P = 64 if scale == 1 else 16
    bs = (1 << 20) if scale == 1 else 30000
    out = {}
    # the class boundaries and MED_CAP: 257, 2048 | 2049, 8192
    out["boundaries"] = ([sized([SM_G + 1, MED_LO_CAP, MED_LO_CAP + 1, MED_CAP], P, 50)], [SM_G + 1, MED_LO_CAP, MED_LO_CAP + 1, MED_CAP], 0)
    # all medium groups in one class (a group loses at most a member per round, and its parts are smaller: the classes hold for every round)
    out["lower_class_only"] = ([sized([300, 1500, MED_LO_CAP], P, 60) + marked(1200, 61)], [300, 1500, MED_LO_CAP, 1200], 0)
    out["upper_class_only"] = ([sized([2100, 5000], P, 70) + marked(3000, 71)], [2100, 5000, 3000], 0)
    # Past-the-end key: the block ends with a stretch. With a key of four symbols the group of residue P - h holds, in the round of
    # offset h, the last copy's member that has exactly h symbols left, and that member looks at the block's end.
    tail = knzlib.corpus().text(20000 if scale == 1 else 3000, 8) + _rnd(P, 80) * 600
    out["block_end"] = ([tail], [600], 4)
    # Two blocks: the first one ends with a stretch (its groups' last members look at the block's end, not into the next block, and the
    # labels of the second block are relative to its own base); the same unit begins the second block.
    first = _rnd(bs - P * 700, 90) + _rnd(P, 91) * 700
    second = _rnd(P, 91) * 500 + knzlib.corpus().text(20000 if scale == 1 else 3000, 9) + _rnd(P, 92) * 2500
    assert len(first) == bs
    out["two_blocks"] = ([first, second], [700, 500, 2500], 4)
    return out


def unsplit(scale):
    """The cases of tests/unsplit_cases.py in the same form (ramp768: unsplit in the round of offset h, split in the round of offset 2h)."""
    return {k: ([d], [], 0) for k, (d, _) in unsplit_cases.build(scale).items()}


def check(name, blocks, sizes):
    """Each input really contains the group sizes it is meant to contain (per block: groups never cross a block's end)."""
    r0 = [round0_sizes(b) for b in blocks]
    for m in sizes:
        assert any(m in s4 and m in s5 for s4, s5 in r0), (name, m)
    medium = sorted(s for s in r0[0][0] | r0[0][1] if s > SM_G)
    if name == "lower_class_only":
        assert medium and all(s <= MED_LO_CAP for s in medium), medium
    if name == "upper_class_only":
        assert medium and all(MED_LO_CAP + 4 < s <= MED_CAP for s in medium), medium      # (+ 4: a member lost per round up to h = P)
    if name in ("block_end", "two_blocks"):
        b = blocks[0]                                    # the suffix with four symbols left is a member of a medium group
        assert SM_G < class_sizes(b, 4)[len(b) - 4] <= MED_CAP, name


_MAJ = re.compile(r"majority path (\d+) \((\d+) members\)")


def rounds(err):
    """The per-round lines the knob bwt_stats prints to stderr -> [(groups worked on, members, all keys equal in, their members,
    majority path, its members)]"""
    st, mj = unsplit_cases.parse_stats(err), [(int(m.group(1)), int(m.group(2))) for m in _MAJ.finditer(err)]
    assert len(st) == len(mj)
    return [s[:4] + m for s, m in zip(st, mj)]
