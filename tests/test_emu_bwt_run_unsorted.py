"""Round 0 without the run members (see tests/run_unsorted_cases.py and tests/test_gpu_bwt_run_unsorted.py) on the CPU: csrc/bwt_fwd.hip
under the fiber emulation (tests/emu/bwt_fwd_emu.cpp compares every block with the oracle), the inputs at emulator size, with the path on
and with the members sent through the sort (KNZ_BWT_RUN_IN_SORT=1), the workgroups dispatched forwards and shuffled. How many members stay
out of the sort is counted from the input (run_unsorted_cases.run_members)."""
import os
import subprocess

import pytest

import run_unsorted_cases
from test_emu_kernels import build, write_case

CASES = run_unsorted_cases.build(0)
KNOBS = ("KNZ_BWT_RUN_IN_SORT", "KNZ_BWT_RUN_FALLBACK", "KNZ_BWT_NO_RUN_ROUND", "KNZ_BWT_RUN_SORT", "KNZ_BWT_NSYM")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build("bwt_fwd_emu", tmp_path_factory.mktemp("run_unsorted"))


def _run(exe, path, blocks, nsym, order, **knobs):
    env = dict(os.environ, KNZ_BWT_STATS="1", HIPEMU_ORDER=order)
    for k in KNOBS:
        env.pop(k, None)
    env.update(knobs)
    if nsym:
        env["KNZ_BWT_NSYM"] = str(nsym)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "OK %d blocks" % len(blocks) in r.stdout, (knobs, order, r.stdout[-2000:] + r.stderr[-2000:])
    lines = run_unsorted_cases.parse(r.stderr)
    assert len(lines) == 1, r.stderr[-2000:]
    return lines[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_members_kept_out_of_the_sort_emulated(exe, tmp_path, name):
    blocks, forced = CASES[name]
    path = str(tmp_path / "case.bin")
    write_case(path, blocks)
    on = [_run(exe, path, blocks, forced, order) for order in ("0", "2")]
    knob = [_run(exe, path, blocks, forced, order, KNZ_BWT_RUN_IN_SORT="1") for order in ("0", "2")]
    print(name, "(nsym, run groups, members, kept out): path on", on[0], "knob", knob[0])
    assert on[0] == on[1] and knob[0] == knob[1], (name, "the order of the workgroups changed the counts")
    nsym = on[0][0]
    want = run_unsorted_cases.run_members(blocks, nsym)
    assert want > 0 and on[0][2] == want and on[0][3] == want, (name, want, on[0])
    assert knob[0][:3] == on[0][:3] and knob[0][3] == 0, (name, knob[0])


@pytest.mark.parametrize("var", ("KNZ_BWT_RUN_FALLBACK", "KNZ_BWT_NO_RUN_ROUND", "KNZ_BWT_RUN_IN_SORT"))
def test_fallbacks_take_the_sort_with_the_members_emulated(exe, tmp_path, var):
    blocks, forced = CASES["batch"]
    path = str(tmp_path / "case.bin")
    write_case(path, blocks)
    line = _run(exe, path, blocks, forced, "2", **{var: "1"})
    assert line[3] == 0, (var, line)
