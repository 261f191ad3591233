"""The run round places the members of its run groups from the run tables alone (csrc/bwt_fwd.hip): k_bwt_f_run_emit writes SA and R of
every member straight to its slot and the member's tie bit into the members' bit map -- a member (run k, R) starts a tie exactly when no
earlier run of k's stretch of equal sort keys is as long as R (k_bwt_f_run_tie_marks) --, and k_bwt_f_run_place<true> reads positions
and bits, finds the member's class in the offsets of the classes, and writes labels and descriptors. No record per member is written.
Round 0 fills a gap (the slots of a run group whose members stayed out of its sort) only within R0_GAP_MARGIN slots of its ends: the
flag kernel's workgroups and the placing kernel's windows that lie inside a gap load no key.

The suffix array of a block is unique, so for every input the BWT output and the stream of the headline chain must be the oracle's, with
the paths on, with the members generated and sorted (knob bwt_run_sort) and with the members sent through round 0's sort (knob
bwt_run_in_sort). Inputs (tests/run_tables_cases.py): stretches of runs that tie, placed where the decision crosses rows of 64 runs, tiles
of RUN_TILE runs and the ends of a segment; classes of just over SM_G members, so that a placement workgroup spans several; gaps of many
margins, of exactly two and of one slot more, at the end of a block's slots and on both sides of a block boundary that no workgroup of
the flag kernel respects; and the inputs of tests/run_direct_cases.py.

That the paths ran is asserted from the "after round 0" line of the knob bwt_stats: the members placed directly are compared with a count
made from the input alone (run_direct_cases.run_members), and the line reports the flag workgroups that lay inside a gap."""
import importlib

import pytest

import run_direct_cases
import run_tables_cases
from test_gpu_parity import gpu_compress

pytestmark = pytest.mark.gpu

CASES = run_tables_cases.build(1)
CHAINS = (("BWT", "NONE"), ("BWT+MTFT+ZRLT", "ANS0"))
SETTINGS = ((), ("bwt_run_sort",), ("bwt_run_in_sort",))          # knobs set to 1


def _lib():
    return importlib.import_module("kanzi_amd.hipapi").lib()


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_members_placed_from_the_run_tables_give_the_oracle_stream(hip, oracle, capfd, name):
    blocks, forced, direct, inside = CASES[name]
    data, bs = b"".join(blocks), (len(blocks[0]) + 15) & ~15                     # (a block size is a multiple of 16)
    assert all(len(b) == bs for b in blocks[:-1]) and len(blocks[-1]) <= bs <= 1 << 20          # the encoder's blocks are the ones counted below
    L = _lib()
    want = {}
    for transform, entropy in CHAINS:
        rc, want[transform] = oracle.compress(data, transform, entropy, bs, headerless=1)
        assert rc == 0
    seen = {}
    try:
        assert L.knz_hip_tune(b"bwt_nsym", run_direct_cases.NSYM if forced else 0) == 0
        for knobs in SETTINGS:
            for k in knobs:
                assert L.knz_hip_tune(k.encode(), 1) == 0
            for transform, entropy in CHAINS:
                stats = transform == "BWT"
                capfd.readouterr()
                assert L.knz_hip_tune(b"bwt_stats", 1 if stats else 0) == 0
                out, bits, hb = gpu_compress(hip, data, transform, entropy, bs, headerless=1)
                assert out == want[transform], (name, transform, knobs)
                if stats:
                    err = capfd.readouterr().err
                    seen[knobs] = (run_direct_cases.parse(err), run_tables_cases.parse_skipped(err))
            for k in knobs:
                assert L.knz_hip_tune(k.encode(), 0) == 0
    finally:
        for k in (b"bwt_stats", b"bwt_run_sort", b"bwt_run_in_sort", b"bwt_nsym"):
            L.knz_hip_tune(k, 0)
    print(name, "([(nsym, run groups, members, placed directly, sorted)], [flag workgroups inside a gap]) per batch:", seen)
    lines, skipped = seen[()]
    assert lines and all(len(v[0]) == len(lines) and len(v[1]) == len(lines) for v in seen.values())
    nsym = lines[0][0]
    assert all(x[0] == nsym for v in seen.values() for x in v[0])
    want_members = run_direct_cases.run_members(blocks, nsym)
    assert want_members > 0 and all(sum(x[2] for x in v[0]) == want_members for v in seen.values()), (name, want_members, seen)
    placed = ((want_members, 0) if direct else (0, want_members))
    assert (sum(x[3] for x in lines), sum(x[4] for x in lines)) == placed, (name, lines)
    assert sum(x[3] for x in seen[("bwt_run_sort",)][0]) == 0 and sum(x[4] for x in seen[("bwt_run_sort",)][0]) == want_members, (name, seen)
    assert (sum(x[3] for x in seen[("bwt_run_in_sort",)][0]), sum(x[4] for x in seen[("bwt_run_in_sort",)][0])) == placed, (name, seen)
    # (the batches of an encode print in any order; without gaps there is nothing to lie inside)
    assert sorted(seen[("bwt_run_sort",)][1]) == sorted(skipped) and sum(seen[("bwt_run_in_sort",)][1]) == 0, (name, seen)
    if inside is not None:
        assert (sum(skipped) > 0) == inside, (name, skipped)
