"""k_bwt_f_medium_fused (see tests/test_gpu_bwt_medium_fused.py) on the CPU: csrc/bwt_fwd.hip under the fiber emulation
(tests/emu/bwt_fwd_emu.cpp compares every block with the oracle). The kernel reads labels in the launch that writes them, which only the
versioned entries make safe: KNZ_EMU's check inside lab_set aborts when a position's label at the round's start is not the `was` the
writer passes, and must stay silent. Inputs of tests/medium_fused_cases.py and tests/unsplit_cases.py at emulator size; the fused path
with the workgroups dispatched forwards and shuffled, with every all-equal group sorted (KNZ_BWT_NO_UNSPLIT_SKIP), and the three
kernels it replaces (KNZ_BWT_NO_MEDIUM_FUSE), which must count the same groups."""
import os
import subprocess

import pytest

import medium_fused_cases
from test_emu_kernels import build, write_case

# (ramp768_one_stretch and text leave the rounds no medium group to speak of: tests/test_emu_bwt_unsplit.py runs them)
CASES = dict({k: v for k, v in medium_fused_cases.unsplit(0).items() if k in ("ramp256", "ramp768", "records", "stretches")}, **medium_fused_cases.build(0))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build("bwt_fwd_emu", tmp_path_factory.mktemp("medium_fused"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_medium_fused_emulated(exe, tmp_path, name):
    blocks, sizes, nsym = CASES[name]
    medium_fused_cases.check(name, blocks, sizes)
    path = str(tmp_path / "case.bin")
    write_case(path, blocks)
    seen = {}
    for setting, order, knob in (("fused", "0", None), ("fused, shuffled", "2", None), ("fused, all sorted", "0", "KNZ_BWT_NO_UNSPLIT_SKIP"),
                                 ("three kernels", "0", "KNZ_BWT_NO_MEDIUM_FUSE")):
        env = dict(os.environ, KNZ_BWT_STATS="1", HIPEMU_ORDER=order)
        if knob:
            env[knob] = "1"
        if nsym:
            env["KNZ_BWT_NSYM"] = str(nsym)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0 and "OK %d blocks" % len(blocks) in r.stdout, (name, setting, r.stdout[-2000:] + r.stderr[-2000:])
        assert "lab_set:" not in r.stderr, (name, setting, r.stderr[-2000:])
        seen[setting] = medium_fused_cases.rounds(r.stderr)
    assert seen["fused"] and seen["fused"] == seen["fused, shuffled"] == seen["three kernels"], name
    assert sum(r[0] for r in seen["fused"]) > 0, name            # the medium path ran
