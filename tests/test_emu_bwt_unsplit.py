"""The unsplit-group path of the forward BWT (see tests/test_gpu_bwt_unsplit.py) on the CPU: csrc/bwt_fwd.hip under the fiber emulation
(tests/emu/bwt_fwd_emu.cpp compares every block with the oracle; KNZ_EMU's lab_set assertion is on), inputs of tests/unsplit_cases.py at
emulator size, with the path on and off (KNZ_BWT_NO_UNSPLIT_SKIP) and the workgroups dispatched forwards and shuffled."""
import os
import subprocess

import pytest

import unsplit_cases
from test_emu_kernels import build, write_case

CASES = unsplit_cases.build(0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build("bwt_fwd_emu", tmp_path_factory.mktemp("unsplit"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_unsplit_medium_groups_emulated(exe, tmp_path, name):
    data, periodic = CASES[name]
    counts, best = unsplit_cases.unsplit_rounds_model(data)
    if periodic:
        assert best >= 2, (name, counts)         # medium groups that stay unsplit for two rounds and more
    path = str(tmp_path / "case.bin")
    write_case(path, [data])
    seen = {}
    for off, order in ((0, "0"), (0, "2"), (1, "0")):
        env = dict(os.environ, KNZ_BWT_STATS="1", HIPEMU_ORDER=order)
        if off:
            env["KNZ_BWT_NO_UNSPLIT_SKIP"] = "1"
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0 and "OK 1 blocks" in r.stdout, (name, off, order, r.stdout[-2000:] + r.stderr[-2000:])
        seen[off] = unsplit_cases.parse_stats(r.stderr)
    assert seen[0] and all(r[4] for r in seen[0]) and not any(r[4] for r in seen[1])
    assert [r[:4] for r in seen[0]] == [r[:4] for r in seen[1]], name
    if periodic:
        assert sum(1 for r in seen[0] if r[2] > 0) >= 2, (name, seen[0])      # the skip path ran, in two rounds at least
