"""The chain round in place (see tests/test_gpu_bwt_chain_fused.py) on the CPU: csrc/bwt_fwd.hip under the fiber
emulation (tests/emu/bwt_fwd_emu.cpp compares every block with the oracle). med_chain_round lays its links, ends and ranks over the
group's own keys and positions in LDS; a barrier missing between a phase that still reads them and the one that overwrites them shows
as a wrong block when the emulator runs the threads of a workgroup one after the other, forwards or shuffled (HIPEMU_ORDER 0 and 2).
KNZ_EMU's check inside lab_set must stay silent. Inputs of tests/chain_fused_cases.py at emulator size (every case fits: the harness
takes a block of any length), inside k_bwt_f_medium_fused and, on plain labels (KNZ_BWT_PLAIN_LABELS), inside k_bwt_f_sort_medium, which
must count the same groups for the chain round."""
import os
import subprocess

import pytest

import chain_fused_cases
from test_emu_kernels import build, write_case

CASES = chain_fused_cases.build(0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build("bwt_fwd_emu", tmp_path_factory.mktemp("chain_fused"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_chain_round_in_place_emulated(exe, tmp_path, name):
    blocks, nsym, period, size, ends = CASES[name]
    chain_fused_cases.check(name, blocks, period, size, ends)
    path = str(tmp_path / "case.bin")
    write_case(path, blocks)
    seen = {}
    for setting, order, knob in (("in place", "0", None), ("in place, shuffled", "2", None), ("plain labels", "0", "KNZ_BWT_PLAIN_LABELS"),
                                 ("plain labels, shuffled", "2", "KNZ_BWT_PLAIN_LABELS")):
        env = dict(os.environ, KNZ_BWT_STATS="1", HIPEMU_ORDER=order)
        if knob:
            env[knob] = "1"
        if nsym:
            env["KNZ_BWT_NSYM"] = str(nsym)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0 and "OK %d blocks" % len(blocks) in r.stdout, (name, setting, r.stdout[-2000:] + r.stderr[-2000:])
        assert "lab_set:" not in r.stderr, (name, setting, r.stderr[-2000:])
        seen[setting] = chain_fused_cases.chain_rounds(r.stderr)
    assert seen["in place"] == seen["in place, shuffled"] == seen["plain labels"] == seen["plain labels, shuffled"], (name, seen)
    assert sum(seen["in place"]) > 0, name                   # the chain round ran
