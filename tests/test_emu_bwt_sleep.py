"""Medium groups that sleep through doubling rounds (k_bwt_f_med_sleep; see tests/test_gpu_bwt_sleep.py) on the CPU: csrc/bwt_fwd.hip under
the fiber emulation (tests/emu/bwt_fwd_emu.cpp compares every block with the oracle; KNZ_EMU's lab_set assertion is on), inputs of
tests/sleep_cases.py at emulator size, with the path on and off (KNZ_BWT_NO_GROUP_SLEEP) and the workgroups dispatched forwards and shuffled.
Which inputs must show sleepers is decided by the CPU model of the rounds (sleep_cases.sleep_rounds_model), not by what the kernels do."""
import os
import subprocess

import pytest

import sleep_cases
import unsplit_cases
from test_emu_kernels import build, write_case

CASES = sleep_cases.build(0)
PERIODIC = ("ramp256", "ramp768", "records", "target_splits")     # (the stretches at this size, period 16, meet the chain round too early)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build("bwt_fwd_emu", tmp_path_factory.mktemp("sleep"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_sleeping_medium_groups_emulated(exe, tmp_path, name):
    data = CASES[name]
    model = sleep_cases.sleep_rounds_model(data)
    predicted = sum(1 for _, _, members in model if members > 0)
    print(name, "model (offset, classes asleep, members asleep):", model)
    if name in PERIODIC:
        assert predicted >= 2, (name, model)
    path = str(tmp_path / "case.bin")
    write_case(path, [data])
    seen = {}
    for off, order in ((0, "0"), (0, "2"), (1, "0")):
        env = dict(os.environ, KNZ_BWT_STATS="1", HIPEMU_ORDER=order)
        env.pop("KNZ_BWT_NO_GROUP_SLEEP", None)
        if off:
            env["KNZ_BWT_NO_GROUP_SLEEP"] = "1"
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0 and "OK 1 blocks" in r.stdout, (name, off, order, r.stdout[-2000:] + r.stderr[-2000:])
        stats = (sleep_cases.parse_sleep(r.stderr), unsplit_cases.parse_stats(r.stderr), sleep_cases.parse_rounds(r.stderr))
        if off in seen:
            assert seen[off] == stats, (name, "the order of the workgroups changed the counts")
        seen[off] = stats
    print(name, "device, asleep per round:", seen[0][0])
    assert seen[0][0] and len(seen[0][0]) == len(seen[1][0])
    assert all(r == (0, 0) for r in seen[1][0]), (name, seen[1][0])              # knob off: nobody sleeps
    assert seen[0][1:] == seen[1][1:], name                                      # rounds, groups and members otherwise the same
    if predicted >= 2:
        assert sum(1 for _, members in seen[0][0] if members > 0) >= 2, (name, model, seen[0][0])
    if name == "run_ties":
        # no group with an override sleeps: what sleeps is at most what the model, which keeps the run ties awake, puts to sleep
        assert sum(m for _, m in seen[0][0]) <= sum(m for _, _, m in model), (name, model, seen[0][0])
