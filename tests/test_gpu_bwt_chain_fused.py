"""The chain round (csrc/bwt_fwd.hip: med_chain_round): a medium group whose majority looks at the group itself is finished by the
workgroup that holds it in LDS, its scratch arrays laid over the group's own keys and positions. The suffix array of a block is unique,
so the headerless device stream must be the oracle's with the round inside k_bwt_f_medium_fused (default), with the fused kernel off
(knob bwt_no_medium_fuse: k_bwt_f_gather_desc + k_bwt_f_sort_medium, the round inside the latter) and with plain labels (knob
bwt_plain_labels: the same two kernels on 32-bit labels, the only way production reaches k_bwt_f_sort_medium, above 256 MiB), and
the rounds' statistics (knob bwt_stats) must count the same groups for the chain round with every setting -- more than none: an input
that never reaches the chain round fails the test.

Inputs: tests/chain_fused_cases.py, blocks of 1 MiB."""
import importlib

import pytest

import chain_fused_cases
from test_gpu_parity import gpu_compress

pytestmark = pytest.mark.gpu

BS = 1 << 20
CASES = chain_fused_cases.build(1)
CHAINS = (("BWT", "NONE"), ("BWT+MTFT+ZRLT", "ANS0"))
# (knob bwt_plain_labels, knob bwt_no_medium_fuse)
SETTINGS = {"in place": (0, 0), "plain labels": (1, 0), "three kernels": (0, 1)}
KNOBS = (b"bwt_stats", b"bwt_plain_labels", b"bwt_no_medium_fuse", b"bwt_nsym")


@pytest.mark.parametrize("name", sorted(CASES))
def test_chain_round_in_place_listed_or_unfused_gives_the_oracle_stream(hip, oracle, capfd, name):
    blocks, nsym, period, size, ends = CASES[name]
    data = b"".join(blocks)
    assert all(len(b) == BS for b in blocks[:-1]) and len(blocks[-1]) <= BS
    chain_fused_cases.check(name, blocks, period, size, ends)
    L = importlib.import_module("kanzi_amd.hipapi").lib()
    want = {}
    for transform, entropy in CHAINS:
        rc, want[transform] = oracle.compress(data, transform, entropy, BS, headerless=1)
        assert rc == 0
    seen = {}
    try:
        assert L.knz_hip_tune(b"bwt_nsym", nsym) == 0
        for setting, (plain_labels, no_fuse) in SETTINGS.items():
            assert L.knz_hip_tune(b"bwt_plain_labels", plain_labels) == 0 and L.knz_hip_tune(b"bwt_no_medium_fuse", no_fuse) == 0
            for transform, entropy in CHAINS:
                stats = transform == "BWT"
                capfd.readouterr()
                assert L.knz_hip_tune(b"bwt_stats", 1 if stats else 0) == 0
                out, bits, hb = gpu_compress(hip, data, transform, entropy, BS, headerless=1)
                assert out == want[transform], (name, transform, setting)
                if stats:
                    seen[setting] = chain_fused_cases.chain_rounds(capfd.readouterr().err)
    finally:
        for knob in KNOBS:
            L.knz_hip_tune(knob, 0)
    for setting in SETTINGS:
        print(name, "%-13s:" % setting, seen[setting])
    assert seen["in place"] == seen["plain labels"] == seen["three kernels"], name
    assert sum(seen["in place"]) > 0, name                   # the chain round ran
