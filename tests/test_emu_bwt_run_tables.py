"""The run round's placement from the run tables and round 0's gaps filled at their ends only (see tests/run_tables_cases.py and
tests/test_gpu_bwt_run_tables.py) on the CPU: csrc/bwt_fwd.hip under the fiber emulation (tests/emu/bwt_fwd_emu.cpp compares every block
with the oracle), the inputs at emulator size. Every case runs with the paths on -- the workgroups dispatched forwards and shuffled --,
with the members generated and sorted (KNZ_BWT_RUN_SORT=1) and with the members sent through round 0's sort (KNZ_BWT_RUN_IN_SORT=1).
That the members were placed directly is read from the statistics line and compared with a count made from the input
(run_direct_cases.run_members); so is the number of flag workgroups that lay inside a gap."""
import os
import subprocess

import pytest

import run_direct_cases
import run_tables_cases
from test_emu_kernels import build, write_case

CASES = run_tables_cases.build(0)
KNOBS = ("KNZ_BWT_RUN_SORT", "KNZ_BWT_RUN_IN_SORT", "KNZ_BWT_RUN_FALLBACK", "KNZ_BWT_NO_RUN_ROUND", "KNZ_BWT_NSYM")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build("bwt_fwd_emu", tmp_path_factory.mktemp("run_tables"))


def _run(exe, path, blocks, forced, order, **knobs):
    env = dict(os.environ, KNZ_BWT_STATS="1", HIPEMU_ORDER=order)
    for k in KNOBS:
        env.pop(k, None)
    env.update(knobs)
    if forced:
        env["KNZ_BWT_NSYM"] = str(run_direct_cases.NSYM)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "OK %d blocks" % len(blocks) in r.stdout, (knobs, order, r.stdout[-2000:] + r.stderr[-2000:])
    lines, skipped = run_direct_cases.parse(r.stderr), run_tables_cases.parse_skipped(r.stderr)
    assert len(lines) == 1 and len(skipped) == 1, r.stderr[-2000:]
    return lines[0], skipped[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_members_placed_from_the_run_tables_emulated(exe, tmp_path, name):
    blocks, forced, direct, inside = CASES[name]
    path = str(tmp_path / "case.bin")
    write_case(path, blocks)
    on = [_run(exe, path, blocks, forced, order) for order in ("0", "2")]
    assert on[0] == on[1], (name, "the order of the workgroups changed the counts")
    sort = _run(exe, path, blocks, forced, "0", KNZ_BWT_RUN_SORT="1")
    in_sort = _run(exe, path, blocks, forced, "0", KNZ_BWT_RUN_IN_SORT="1")
    print(name, "((nsym, run groups, members, placed directly, sorted), flag workgroups inside a gap): paths on", on[0], "members sorted", sort,
          "members in round 0's sort", in_sort)
    (nsym, _, members, placed, sorted_), skipped = on[0]
    want = run_direct_cases.run_members(blocks, nsym)
    assert want > 0 and members == want, (name, want, on[0])
    assert (placed, sorted_) == ((want, 0) if direct else (0, want)), (name, on[0])
    assert sort[0][:3] == on[0][0][:3] and sort[0][3:] == (0, want) and sort[1] == skipped, (name, sort)
    assert in_sort[0] == on[0][0] and in_sort[1] == 0, (name, in_sort)          # (no gaps: nothing to lie inside)
    if inside is not None:
        assert (skipped > 0) == inside, (name, skipped)
