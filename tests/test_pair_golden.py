"""Pins tests/golden/pairs.json (tools/make_pair_golden.py) to the reference build: the input, the digest of every case the file
records, the condition on what it may leave out, and that the input makes every stage that can refuse a block do both."""
import hashlib
import json
import os

import pytest

import pair_cases as cases

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairs.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


@pytest.fixture(scope="module")
def data():
    d = cases.make_input()
    assert len(d) == GOLDEN["n"] == cases.N and md5(d) == GOLDEN["input_md5"]
    return d


def test_input_is_the_recorded_one(data):
    assert GOLDEN["block_size"] == cases.BS
    assert len(data) % cases.BS == 10              # nine whole blocks and a copy block


@pytest.mark.parametrize("ps", cases.PASSES)
def test_only_the_zrlt_family_is_left_out(ps):
    """At most five cases per pass, and only chains whose second stage is ZRLT: the reference alone meets this on this input."""
    recs = cases.records(GOLDEN, ps)
    left = [r["chain"] for r in recs if "left_out" in r]
    assert len(left) <= cases.MAX_LEFT_OUT, left
    assert all(c.split("+")[1] == "ZRLT" for c in left), left
    assert all(r["left_out"] for r in recs if "left_out" in r)          # with its reason
    if ps == "B":                                                       # every stage meets every coder, in first and in second position
        for pos in (0, 1):
            assert {(r["chain"].split("+")[pos], r["entropy"]) for r in recs} == {(t, e) for t in cases.T for e in cases.E}
        assert {r["checksum"] for r in recs} == {0, 32, 64} and {r["jobs"] for r in recs} == {1, 2, 3}


@pytest.mark.parametrize("ps", cases.PASSES)
def test_recorded_digests_are_the_references(ref, data, ps):
    """Every case that is not left out, computed again (the cases left out corrupt the reference's heap and are never run)."""
    n = 0
    for r in cases.records(GOLDEN, ps):
        if "left_out" in r:
            continue
        rc, knz = ref.compress(data, r["chain"], r["entropy"], cases.BS, jobs=r["jobs"], checksum=r["checksum"], orig_size=len(data))
        assert rc == 0, r
        assert (len(knz), md5(knz)) == (r["knz_len"], r["knz_md5"]), r
        n += 1
    assert n >= 14 * 14 - cases.MAX_LEFT_OUT


@pytest.mark.parametrize("stage", cases.MAY_REFUSE)
def test_every_refusing_stage_accepts_and_refuses(ref, data, stage):
    """Alone on the nine whole blocks, with the capacity a stream gives it: the stage takes at least one block and refuses at least one,
    so behind it both a transformed and an untouched block reach the second stage of a pair."""
    taken = 0
    for b in range(9):
        blk = data[b * cases.BS:(b + 1) * cases.BS]
        ok, _, skip = ref.forward(stage, blk, len(blk) + 2048)
        assert ok in (0, 1) and bool(skip & 0x80) == (ok == 0), (stage, b, ok, skip)
        taken += ok
    assert 1 <= taken <= 8, (stage, taken)
