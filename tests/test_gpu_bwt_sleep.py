"""Medium groups sleep through the doubling rounds whose verdict is known from the round before (k_bwt_f_med_sleep, csrc/bwt_fwd.hip): when
all members of G found G' h positions on, all members of G' found G'', and G'' came out of that round whole, every member of G finds G''
2h positions on -- the group is staged again without a member being read. The suffix array of a block is unique, so the streams must be the
oracle's with the path on and with it off (knob bwt_no_group_sleep). Inputs (tests/sleep_cases.py): ramps of period 256 and 768, records
with a shared prefix, periodic stretches, run ties (medium groups with an override, which never sleep), records whose target group splits
while they are still whole (the sleeper must be gathered that round), text (nothing sleeps).

That the path ran is asserted from the counters (knob bwt_stats), on the inputs for which the CPU model of the rounds
(sleep_cases.sleep_rounds_model) predicts two sleeping rounds and more; an input for which it predicts none is a negative case."""
import importlib

import pytest

import sleep_cases
import unsplit_cases
from test_gpu_parity import gpu_compress

pytestmark = pytest.mark.gpu

BS = 1 << 20
CASES = sleep_cases.build(1)
PERIODIC = ("ramp256", "ramp768", "records", "stretches", "target_splits")


@pytest.mark.parametrize("name", sorted(CASES))
def test_sleeping_medium_groups_give_the_oracle_stream(hip, oracle, capfd, name):
    data = CASES[name]
    assert len(data) <= BS                       # one block: the CPU model below sees what the device sorts
    model = sleep_cases.sleep_rounds_model(data)
    predicted = sum(1 for _, _, members in model if members > 0)
    print(name, "model (offset, classes asleep, members asleep):", model)
    if name in PERIODIC:
        assert predicted >= 2, (name, model)
    L = importlib.import_module("kanzi_amd.hipapi").lib()
    want = {}
    for transform, entropy in (("BWT", "NONE"), ("BWT+MTFT+ZRLT", "ANS0")):
        rc, want[transform] = oracle.compress(data, transform, entropy, BS, headerless=1)
        assert rc == 0
    seen = {}
    try:
        for off in (0, 1):
            assert L.knz_hip_tune(b"bwt_no_group_sleep", off) == 0
            for transform, entropy in (("BWT", "NONE"), ("BWT+MTFT+ZRLT", "ANS0")):
                stats = transform == "BWT"
                capfd.readouterr()
                assert L.knz_hip_tune(b"bwt_stats", 1 if stats else 0) == 0
                out, bits, hb = gpu_compress(hip, data, transform, entropy, BS, headerless=1)
                assert out == want[transform], (name, transform, "sleep off" if off else "sleep on")
                if stats:
                    err = capfd.readouterr().err
                    seen[off] = (sleep_cases.parse_sleep(err), unsplit_cases.parse_stats(err), sleep_cases.parse_rounds(err))
    finally:
        L.knz_hip_tune(b"bwt_stats", 0)
        L.knz_hip_tune(b"bwt_no_group_sleep", 0)
    print(name, "device, asleep per round, sleep on :", seen[0][0])
    print(name, "device, asleep per round, sleep off:", seen[1][0])
    assert seen[0][0] and len(seen[0][0]) == len(seen[1][0])
    assert all(r == (0, 0) for r in seen[1][0]), (name, seen[1][0])              # knob off: nobody sleeps
    assert seen[0][1:] == seen[1][1:], name                                      # rounds, groups and members otherwise the same
    if predicted >= 2:
        assert sum(1 for _, members in seen[0][0] if members > 0) >= 2, (name, model, seen[0][0])
    if name == "run_ties":
        # no group with an override sleeps: what sleeps is at most what the model, which keeps the run ties awake, puts to sleep
        assert sum(m for _, m in seen[0][0]) <= sum(m for _, _, m in model), (name, model, seen[0][0])
