"""The forward BWT's alternate ways through the run round and the link step (csrc/bwt_fwd.hip), which production takes by itself on some
batches and which so far ran under the emulator only:

  * k_bwt_f_run_fallback, the run groups handed to the ordinary rounds: taken when a batch has more run groups than the run key has index
    bits, or more runs than the tables hold (a round-0 key of fewer than 4 symbols: knob bwt_nsym 3), and under the knob bwt_run_fallback;
  * no run round at all (knob bwt_no_run_round);
  * the link step for small groups inside long repeats off (bwt_link 0) and tried from the first doubling round on (bwt_link 4).

The suffix array of a block is unique, so with every setting the headerless BWT / NONE stream is the oracle's. The kernel times and the
rounds' statistics (knob bwt_stats, on stderr) say that the path was taken. Blocks of 1 MiB; inputs from tests/run_direct_cases.py, and
text with copied spans, X || X and a text followed by itself with two edits (as tests/test_emu_kernels.py has them for the emulator)."""
import importlib

import numpy as np
import pytest

import knzlib
import run_direct_cases
from test_gpu_parity import gpu_compress

pytestmark = pytest.mark.gpu

BS = 1 << 20
KNOBS = {b"bwt_stats": 0, b"bwt_nsym": 0, b"bwt_run_fallback": 0, b"bwt_no_run_round": 0, b"bwt_link": 1}        # knob -> default
SETTINGS = {
    "defaults": {},
    "run_fallback": {b"bwt_run_fallback": 1},
    "no_run_round": {b"bwt_no_run_round": 1},
    "nsym_3": {b"bwt_nsym": 3},
    "link_0": {b"bwt_link": 0},
    "link_4": {b"bwt_link": 4},
}


def runs_of_three():
    """Runs of exactly three bytes of four symbols, no two neighbours alike: a third of the positions start a run of at least 3, more than
    the run tables hold (a quarter: runs of at least 4 symbols) -- with a round-0 key of 3 symbols the run round finds that out and
    falls back; with the default key there is no run group at all."""
    rng = np.random.default_rng(61)
    sym = rng.integers(1, 4, BS // 3 + 1)
    return bytes(np.repeat((np.cumsum(sym) % 4 + 100).astype(np.uint8), 3)[:BS])


def copies():
    c = knzlib.corpus()
    t = c.text(BS // 2, 9)
    ed = bytearray(t); ed[777] = 1; ed[222222] = 2
    return c.repeats(BS, 3) + c.tile(BS, 1, BS // 2) + t + bytes(ed)


def inputs():
    """name -> (data, nsym the synthetic inputs are sorted with (0: by the data), has run groups under the defaults)"""
    rd = run_direct_cases.build(1)
    out = {name: (b"".join(rd[name][0]), run_direct_cases.NSYM if rd[name][1] else 0, True)
           for name in ("both_directions", "multi_tile", "long_run_above_limit", "batch", "mixed")}
    out["runs_of_three"] = (runs_of_three(), 0, False)
    out["copies"] = (copies(), 0, False)
    return out


INPUTS = inputs()


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_run_and_link_paths_give_the_oracle_stream(hip, oracle, capfd, name):
    data, nsym, has_runs = INPUTS[name]
    L = importlib.import_module("kanzi_amd.hipapi").lib()
    rc, want = oracle.compress(data, "BWT", "NONE", BS, headerless=1)
    assert rc == 0
    ran, err, groups = {}, {}, {}
    try:
        for setting, knobs in SETTINGS.items():
            for knob, default in KNOBS.items():
                assert L.knz_hip_tune(knob, knobs.get(knob, nsym if knob == b"bwt_nsym" else default)) == 0
            assert L.knz_hip_tune(b"bwt_stats", 1) == 0
            capfd.readouterr()
            hip.set_profiling(True)
            try:
                out, bits, hb = gpu_compress(hip, data, "BWT", "NONE", BS, headerless=1)
                ran[setting] = {k: launches for k, ms, launches in hip.kernel_times()}
            finally:
                hip.set_profiling(False)
            err[setting] = capfd.readouterr().err
            assert out == want, (name, setting)
            groups[setting] = sum(g for _, g, _, _, _ in run_direct_cases.parse(err[setting]))
    finally:
        for knob, default in KNOBS.items():
            L.knz_hip_tune(knob, default)
    for setting in SETTINGS:
        print(name, "%-13s: run groups after round 0 %d, k_bwt_f_run_fallback %d, k_bwt_f_run_ends %d, link step %s" % (
            setting, groups[setting], ran[setting].get("k_bwt_f_run_fallback", 0), ran[setting].get("k_bwt_f_run_ends", 0),
            "link step:" in err[setting]))

    def launches(setting, kernel):
        return ran[setting].get(kernel, 0)
    # by default no input here goes the ordinary way with its run groups; under the knob every input with run groups does
    assert launches("defaults", "k_bwt_f_run_fallback") == 0, name
    assert launches("no_run_round", "k_bwt_f_run_ends") == 0 and launches("no_run_round", "k_bwt_f_run_fallback") == 0, name
    if has_runs:
        assert groups["defaults"] > 0 and launches("defaults", "k_bwt_f_run_ends") > 0, name         # the run round ran
        assert launches("run_fallback", "k_bwt_f_run_fallback") > 0 and launches("run_fallback", "k_bwt_f_run_ends") == 0, name
        assert groups["run_fallback"] == 0 and groups["no_run_round"] == 0, name                     # (the groups went to the ordinary rounds)
    if name == "runs_of_three":
        # the other way into the fall-back: the run round starts, counts more runs than its tables hold and hands the groups on
        assert groups["defaults"] == 0 and launches("nsym_3", "k_bwt_f_run_ends") > 0 and launches("nsym_3", "k_bwt_f_run_fallback") > 0
    if name == "copies":
        assert "link step:" in err["link_4"] and "link step:" not in err["link_0"]
