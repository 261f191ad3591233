"""The run round places the members of its run groups directly (k_bwt_f_run_emit, csrc/bwt_fwd.hip): the sorted order of the members of
one (byte, direction) is a ragged matrix read column by column, so a member's slot is three counts over the runs and nobody sorts the
members. The suffix array of a block is unique, so the BWT output and the stream of the headline chain must be the oracle's with the path
on and with the members generated and sorted as before (knob bwt_run_sort). Inputs (tests/run_direct_cases.py): runs of every length in
both directions, repeated stretches whose members tie, a segment of four tiles, segments of exactly RUN_TILE and RUN_TILE + 1 runs, a
run just below and one just above RUN_DIRECT_LMAX (above it the batch is sorted), a block of one byte, a batch of blocks whose bytes
repeat from block to block, and the start of the mixed stand-in.

That the path ran is asserted from the "after round 0" line of the knob bwt_stats, whose member counts are compared with a count made
from the input alone (run_direct_cases.run_members)."""
import importlib

import pytest

import run_direct_cases
from test_gpu_parity import gpu_compress, gpu_decompress

pytestmark = pytest.mark.gpu

CASES = run_direct_cases.build(1)


def _lib():
    return importlib.import_module("kanzi_amd.hipapi").lib()


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_members_placed_directly_give_the_oracle_stream(hip, oracle, capfd, name):
    blocks, forced, direct = CASES[name]
    data, bs = b"".join(blocks), (len(blocks[0]) + 15) & ~15                     # (a block size is a multiple of 16)
    assert all(len(b) == bs for b in blocks[:-1]) and len(blocks[-1]) <= bs          # the encoder's blocks are the ones counted below
    L = _lib()
    chains = (("BWT", "NONE"), ("BWT+MTFT+ZRLT", "ANS0"))
    want = {}
    for transform, entropy in chains:
        rc, want[transform] = oracle.compress(data, transform, entropy, bs, headerless=1)
        assert rc == 0
    seen = {}
    try:
        assert L.knz_hip_tune(b"bwt_nsym", run_direct_cases.NSYM if forced else 0) == 0
        for sort in (0, 1):
            assert L.knz_hip_tune(b"bwt_run_sort", sort) == 0
            for transform, entropy in chains:
                stats = transform == "BWT"
                capfd.readouterr()
                assert L.knz_hip_tune(b"bwt_stats", 1 if stats else 0) == 0
                out, bits, hb = gpu_compress(hip, data, transform, entropy, bs, headerless=1)
                assert out == want[transform], (name, transform, "members sorted" if sort else "members placed directly")
                if stats:
                    seen[sort] = run_direct_cases.parse(capfd.readouterr().err)
    finally:
        L.knz_hip_tune(b"bwt_stats", 0)
        L.knz_hip_tune(b"bwt_run_sort", 0)
        L.knz_hip_tune(b"bwt_nsym", 0)
    print(name, "(nsym, run groups, members, placed directly, sorted) per batch: path on", seen[0], "knob", seen[1])
    assert seen[0] and len(seen[0]) == len(seen[1])
    nsym = seen[0][0][0]
    assert all(line[0] == nsym for line in seen[0] + seen[1])
    want_members = run_direct_cases.run_members(blocks, nsym)
    placed, sorted_ = sum(x[3] for x in seen[0]), sum(x[4] for x in seen[0])
    assert want_members > 0 and sum(x[2] for x in seen[0]) == want_members and placed + sorted_ == want_members, (name, want_members, seen[0])
    assert (placed, sorted_) == ((want_members, 0) if direct else (0, want_members)), (name, seen[0])
    assert sum(x[3] for x in seen[1]) == 0 and sum(x[4] for x in seen[1]) == want_members, (name, seen[1])


def test_bwts_chain_with_run_members_placed_directly(hip, capfd):
    """BWTS shares the suffix sort: its output and the stream of BWTS+MTFT+ZRLT in front of ANS0 are the same with the path on and with
    the knob, the path ran (statistics line), and both decode to the input (the inverse is checked against the reference elsewhere)."""
    blocks, _, _ = CASES["both_directions"]
    data = blocks[0]
    L = _lib()
    got = {}
    try:
        assert L.knz_hip_tune(b"bwt_nsym", run_direct_cases.NSYM) == 0
        for sort in (0, 1):
            assert L.knz_hip_tune(b"bwt_run_sort", sort) == 0
            capfd.readouterr()
            assert L.knz_hip_tune(b"bwt_stats", 1) == 0
            ok, fwd = hip.transform_forward("BWTS", data, len(data))
            assert L.knz_hip_tune(b"bwt_stats", 0) == 0
            lines = run_direct_cases.parse(capfd.readouterr().err)
            assert ok and lines and sum(x[3] for x in lines) + sum(x[4] for x in lines) > 0
            assert (sum(x[4] for x in lines) == 0) == (sort == 0), lines
            bs = (len(data) + 15) & ~15
            out, bits, hb = gpu_compress(hip, data, "BWTS+MTFT+ZRLT", "ANS0", bs, headerless=1)
            got[sort] = (fwd, out)
            ok, back = hip.transform_inverse("BWTS", fwd, len(data))
            assert ok and back == data
            assert gpu_decompress(hip, out, "BWTS+MTFT+ZRLT", "ANS0", bs, len(data), 0) == data
    finally:
        L.knz_hip_tune(b"bwt_stats", 0)
        L.knz_hip_tune(b"bwt_run_sort", 0)
        L.knz_hip_tune(b"bwt_nsym", 0)
    assert got[0] == got[1]
