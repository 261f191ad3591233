"""The run round's direct placement of the run members (k_bwt_f_run_emit; see tests/test_gpu_bwt_run_direct.py) on the CPU:
csrc/bwt_fwd.hip under the fiber emulation (tests/emu/bwt_fwd_emu.cpp compares every block with the oracle), inputs of
tests/run_direct_cases.py at emulator size, with the path on and off (KNZ_BWT_RUN_SORT=1: the members generated and sorted) and the
workgroups dispatched forwards and shuffled. How many members there are is counted from the input (run_direct_cases.run_members)."""
import os
import subprocess

import pytest

import run_direct_cases
from test_emu_kernels import build, write_case

CASES = run_direct_cases.build(0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build("bwt_fwd_emu", tmp_path_factory.mktemp("run_direct"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_members_placed_directly_emulated(exe, tmp_path, name):
    blocks, forced, direct = CASES[name]
    path = str(tmp_path / "case.bin")
    write_case(path, blocks)
    seen = {}
    for sort, order in ((0, "0"), (0, "2"), (1, "0")):
        env = dict(os.environ, KNZ_BWT_STATS="1", HIPEMU_ORDER=order)
        for k in ("KNZ_BWT_RUN_SORT", "KNZ_BWT_NSYM"):
            env.pop(k, None)
        if sort:
            env["KNZ_BWT_RUN_SORT"] = "1"
        if forced:
            env["KNZ_BWT_NSYM"] = str(run_direct_cases.NSYM)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0 and "OK %d blocks" % len(blocks) in r.stdout, (name, sort, order, r.stdout[-2000:] + r.stderr[-2000:])
        lines = run_direct_cases.parse(r.stderr)
        assert len(lines) == 1, (name, r.stderr[-2000:])
        if sort in seen:
            assert seen[sort] == lines[0], (name, "the order of the workgroups changed the counts")
        seen[sort] = lines[0]
    print(name, "(nsym, run groups, members, placed directly, sorted): path on", seen[0], "knob", seen[1])
    nsym, _, members, placed, sorted_ = seen[0]
    want = run_direct_cases.run_members(blocks, nsym)
    assert want > 0 and members == want and placed + sorted_ == want, (name, want, seen[0])
    assert (placed, sorted_) == ((want, 0) if direct else (0, want)), (name, seen[0])
    assert seen[1][:3] == seen[0][:3] and seen[1][3:] == (0, want), (name, seen[1])
