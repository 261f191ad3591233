"""Round 0 of the forward suffix sort keeps the run members out of its sort (csrc/bwt_fwd.hip: FwdSort::run_scan finds the run groups in
the text before anything is sorted, the first pass drops their members, the last pass leaves a gap per group, k_bwt_f_r0_fill puts one key
into it, and the run round writes every member). The suffix array of a block is unique, so the BWT output and the stream of the headline
chain must be the oracle's with the path on and with the members sent through the sort as before (knob bwt_run_in_sort). Inputs
(tests/run_unsorted_cases.py): a class of exactly SM_G members beside one of SM_G + 1, a block of one byte, a block of two runs, blocks
that end in a run of zeros and of another byte, runs followed by a run of another class, by a byte without a class and by the block end,
a tile of the first pass that holds members only and one with a single other element, both key lengths, a run above RUN_DIRECT_LMAX, a
batch of blocks with different classes and none, and the first 256 KiB of every segment kind of the mixed stand-in.

That the path ran is asserted from the "after round 0" line of the knob bwt_stats: the members kept out of the sort are compared with a
count made from the input alone (run_unsorted_cases.run_members), and must be 0 wherever a knob sends the batch the old way."""
import importlib

import pytest

import run_unsorted_cases
from test_gpu_parity import gpu_compress, gpu_decompress

pytestmark = pytest.mark.gpu

CASES = run_unsorted_cases.build(1)
CHAINS = (("BWT", "NONE"), ("BWT+MTFT+ZRLT", "ANS0"))


def _lib():
    return importlib.import_module("kanzi_amd.hipapi").lib()


def _block_size(blocks):
    bs = (len(blocks[0]) + 15) & ~15                                                # (a block size is a multiple of 16)
    assert all(len(b) == bs for b in blocks[:-1]) and len(blocks[-1]) <= bs          # the encoder's blocks are the ones counted
    return bs


@pytest.fixture(scope="module")
def oracle_streams(oracle):
    """name -> chain -> the oracle's stream, computed once"""
    want = {}
    for name, (blocks, _) in CASES.items():
        data, bs = b"".join(blocks), _block_size(blocks)
        want[name] = {}
        for transform, entropy in CHAINS:
            rc, want[name][transform] = oracle.compress(data, transform, entropy, bs, headerless=1)
            assert rc == 0
    return want


def _encode_all(hip, capfd, L, data, bs, want, tag):
    """both chains against the oracle; the statistics lines of the BWT / NONE encode"""
    lines = None
    for transform, entropy in CHAINS:
        stats = transform == "BWT"
        capfd.readouterr()
        assert L.knz_hip_tune(b"bwt_stats", 1 if stats else 0) == 0
        out, bits, hb = gpu_compress(hip, data, transform, entropy, bs, headerless=1)
        assert out == want[transform], (tag, transform)
        if stats:
            lines = run_unsorted_cases.parse(capfd.readouterr().err)
    return lines


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_members_kept_out_of_the_sort_give_the_oracle_stream(hip, oracle_streams, capfd, name):
    blocks, forced = CASES[name]
    data, bs = b"".join(blocks), _block_size(blocks)
    L = _lib()
    seen = {}
    try:
        assert L.knz_hip_tune(b"bwt_nsym", forced) == 0
        for knob in (0, 1):
            assert L.knz_hip_tune(b"bwt_run_in_sort", knob) == 0
            seen[knob] = _encode_all(hip, capfd, L, data, bs, oracle_streams[name], (name, "members in the sort" if knob else "members kept out"))
    finally:
        L.knz_hip_tune(b"bwt_stats", 0)
        L.knz_hip_tune(b"bwt_run_in_sort", 0)
        L.knz_hip_tune(b"bwt_nsym", 0)
    print(name, "(nsym, run groups, members, kept out) per batch: path on", seen[0], "knob", seen[1])
    assert seen[0] and len(seen[0]) == len(seen[1])
    nsym = seen[0][0][0]
    assert all(line[0] == nsym for line in seen[0] + seen[1])
    want_members = run_unsorted_cases.run_members(blocks, nsym)
    assert want_members > 0 and sum(x[2] for x in seen[0]) == want_members and sum(x[3] for x in seen[0]) == want_members, (name, want_members, seen[0])
    assert sum(x[2] for x in seen[1]) == want_members and sum(x[3] for x in seen[1]) == 0, (name, seen[1])


@pytest.mark.parametrize("knob", ("bwt_run_fallback", "bwt_no_run_round", "bwt_run_in_sort"))
def test_fallbacks_send_the_members_through_the_sort(hip, oracle_streams, capfd, knob):
    blocks, forced = CASES["batch"]
    data, bs = b"".join(blocks), _block_size(blocks)
    L = _lib()
    try:
        assert L.knz_hip_tune(b"bwt_nsym", forced) == 0
        assert L.knz_hip_tune(knob.encode(), 1) == 0
        lines = _encode_all(hip, capfd, L, data, bs, oracle_streams["batch"], knob)
    finally:
        L.knz_hip_tune(b"bwt_stats", 0)
        L.knz_hip_tune(knob.encode(), 0)
        L.knz_hip_tune(b"bwt_nsym", 0)
    assert lines and sum(x[3] for x in lines) == 0, (knob, lines)


def test_bwts_chain_with_run_members_kept_out_of_the_sort(hip, capfd):
    """BWTS shares the suffix sort: its output and the stream of BWTS+MTFT+ZRLT in front of ANS0 are the same with the path on and with
    the knob, the path ran (statistics line), and both decode to the input (the inverse is checked against the reference elsewhere)."""
    blocks, forced = CASES["behind_class"]
    data = blocks[0]
    L = _lib()
    got = {}
    try:
        assert L.knz_hip_tune(b"bwt_nsym", forced) == 0
        for knob in (0, 1):
            assert L.knz_hip_tune(b"bwt_run_in_sort", knob) == 0
            capfd.readouterr()
            assert L.knz_hip_tune(b"bwt_stats", 1) == 0
            ok, fwd = hip.transform_forward("BWTS", data, len(data))
            assert L.knz_hip_tune(b"bwt_stats", 0) == 0
            lines = run_unsorted_cases.parse(capfd.readouterr().err)
            assert ok and lines and sum(x[2] for x in lines) > 0
            assert sum(x[3] for x in lines) == (0 if knob else sum(x[2] for x in lines)), lines
            bs = (len(data) + 15) & ~15
            out, bits, hb = gpu_compress(hip, data, "BWTS+MTFT+ZRLT", "ANS0", bs, headerless=1)
            got[knob] = (fwd, out)
            ok, back = hip.transform_inverse("BWTS", fwd, len(data))
            assert ok and back == data
            assert gpu_decompress(hip, out, "BWTS+MTFT+ZRLT", "ANS0", bs, len(data), 0) == data
    finally:
        L.knz_hip_tune(b"bwt_stats", 0)
        L.knz_hip_tune(b"bwt_run_in_sort", 0)
        L.knz_hip_tune(b"bwt_nsym", 0)
    assert got[0] == got[1]
