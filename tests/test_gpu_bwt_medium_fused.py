"""k_bwt_f_medium_fused (csrc/bwt_fwd.hip): with versioned labels one workgroup fetches a medium group's keys, judges them and sorts the
group; keys go neither through K nor through descInfo, and each of the two launches is dealt the groups of its size class only. The
suffix array of a block is unique, so the headerless device stream must be the oracle's with the fused path on, with it off (knob
bwt_no_medium_fuse: k_bwt_f_gather_desc + k_bwt_f_sort_medium) and with every all-equal group sorted (bwt_no_unsplit_skip), and the
rounds' statistics (knob bwt_stats) must count the same groups with the path on and off.

Inputs (tests/medium_fused_cases.py, blocks of 1 MiB): the cases of tests/unsplit_cases.py -- ramp768 is the group that is unsplit in the
round of offset h and splits in the round of offset 2h -- and groups of exactly 257, 2048, 2049 and 8192 members (class boundaries,
MED_CAP), blocks whose medium groups all belong to one class (the other class's launch is left out), a group at a block's end whose
members look past the end, and two blocks in one batch."""
import importlib

import pytest

import knzlib
import medium_fused_cases
import unsplit_cases
from test_gpu_parity import gpu_compress

pytestmark = pytest.mark.gpu

BS = 1 << 20
CASES = dict(medium_fused_cases.unsplit(1), **medium_fused_cases.build(1))
CHAINS = (("BWT", "NONE"), ("BWT+MTFT+ZRLT", "ANS0"))
# (knob bwt_no_medium_fuse, knob bwt_no_unsplit_skip)
SETTINGS = {"fused": (0, 0), "three kernels": (1, 0), "fused, all-equal groups sorted": (0, 1)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_medium_groups_fused_or_not_give_the_oracle_stream(hip, oracle, capfd, name):
    blocks, sizes, nsym = CASES[name]
    data = b"".join(blocks)
    assert all(len(b) == BS for b in blocks[:-1]) and len(blocks[-1]) <= BS
    medium_fused_cases.check(name, blocks, sizes)
    if name == "ramp768":
        counts, best = unsplit_cases.unsplit_rounds_model(data)
        print(name, "model: unsplit medium classes per round", counts, "longest stay", best)
        assert best >= 2 and counts[0] > counts[-1], counts      # groups whole in one round and split in a later one
    L = importlib.import_module("kanzi_amd.hipapi").lib()
    want = {}
    for transform, entropy in CHAINS:
        rc, want[transform] = oracle.compress(data, transform, entropy, BS, headerless=1)
        assert rc == 0
    seen = {}
    try:
        assert L.knz_hip_tune(b"bwt_nsym", nsym) == 0
        for setting, (no_fuse, no_skip) in SETTINGS.items():
            assert L.knz_hip_tune(b"bwt_no_medium_fuse", no_fuse) == 0 and L.knz_hip_tune(b"bwt_no_unsplit_skip", no_skip) == 0
            for transform, entropy in CHAINS:
                stats = transform == "BWT" and not no_skip
                capfd.readouterr()
                assert L.knz_hip_tune(b"bwt_stats", 1 if stats else 0) == 0
                out, bits, hb = gpu_compress(hip, data, transform, entropy, BS, headerless=1)
                assert out == want[transform], (name, transform, setting)
                if stats:
                    seen[setting] = medium_fused_cases.rounds(capfd.readouterr().err)
    finally:
        for knob in (b"bwt_stats", b"bwt_no_medium_fuse", b"bwt_no_unsplit_skip", b"bwt_nsym"):
            L.knz_hip_tune(knob, 0)
    print(name, "fused        :", seen["fused"])
    print(name, "three kernels:", seen["three kernels"])
    assert seen["fused"] and seen["fused"] == seen["three kernels"], name
    if sizes:
        assert sum(r[0] for r in seen["fused"]) > 0, name        # the medium path ran
