"""Medium groups a doubling round cannot split (all members carry one key) are neither stored nor sorted: k_bwt_f_gather_desc sees it
while it holds the group's keys in registers, stages the group for the next round and voids the round's descriptor. The suffix array of a
block is unique, so the streams must be the oracle's with the path on and with it off (knob bwt_no_unsplit_skip). Inputs are built here
(tests/unsplit_cases.py): ramps of period 256 and 768, records with a shared prefix, periodic stretches of 6,000 and 9,000 members per
residue (a two-batch medium group; large groups above MED_CAP), text.

A group that is unsplit in the round of offset h and splits in the round of offset 2h must come out right: the period-768 ramp is that case
(no offset meets the period, its groups lose the members near a stretch's end round by round), and so are the records (a group per prefix
offset, whole until the offset reaches the random tails)."""
import importlib

import pytest

import knzlib
import unsplit_cases
from test_gpu_parity import gpu_compress

pytestmark = pytest.mark.gpu

BS = 1 << 20
CASES = unsplit_cases.build(1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_unsplit_medium_groups_skipped_or_sorted_give_the_oracle_stream(hip, oracle, capfd, name):
    data, periodic = CASES[name]
    assert len(data) <= BS                       # one block: the CPU model below sees what the device sorts
    counts, best = unsplit_cases.unsplit_rounds_model(data)
    print(name, "model: unsplit medium classes per round", counts, "longest stay", best)
    if periodic:
        assert best >= 2, (name, counts)         # the input really has medium groups that stay unsplit for two rounds and more
    L = importlib.import_module("kanzi_amd.hipapi").lib()
    want = {}
    for transform, entropy in (("BWT", "NONE"), ("BWT+MTFT+ZRLT", "ANS0")):
        rc, want[transform] = oracle.compress(data, transform, entropy, BS, headerless=1)
        assert rc == 0
    seen = {}
    try:
        for off in (0, 1):
            assert L.knz_hip_tune(b"bwt_no_unsplit_skip", off) == 0
            for transform, entropy in (("BWT", "NONE"), ("BWT+MTFT+ZRLT", "ANS0")):
                stats = transform == "BWT"
                capfd.readouterr()
                assert L.knz_hip_tune(b"bwt_stats", 1 if stats else 0) == 0
                out, bits, hb = gpu_compress(hip, data, transform, entropy, BS, headerless=1)
                assert out == want[transform], (name, transform, "skip off" if off else "skip on")
                if stats:
                    seen[off] = unsplit_cases.parse_stats(capfd.readouterr().err)
    finally:
        L.knz_hip_tune(b"bwt_stats", 0)
        L.knz_hip_tune(b"bwt_no_unsplit_skip", 0)
    print(name, "device, skip on :", seen[0])
    print(name, "device, skip off:", seen[1])
    assert seen[0] and all(r[4] for r in seen[0]) and not any(r[4] for r in seen[1])
    # the verdict of the gather kernel (skip on) names the groups the sorting kernel finds with all keys equal (skip off)
    assert [r[:4] for r in seen[0]] == [r[:4] for r in seen[1]], name
    if periodic:
        assert sum(1 for r in seen[0] if r[2] > 0) >= 2, (name, seen[0])      # the skip path ran, in two rounds at least
