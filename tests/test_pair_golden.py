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


# ---- the typed table: EXE, TEXT and DNA in front of and behind all 17 stages (tests/golden/pairs_typed.json)

GOLDEN_TYPED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairs_typed.json")))
NEW = cases.T_TYPED[14:]


@pytest.fixture(scope="module")
def typed():
    d = cases.make_typed_input()
    assert len(d) == GOLDEN_TYPED["n"] == cases.N_TYPED and md5(d) == GOLDEN_TYPED["input_md5"]
    return d


def test_typed_input_is_the_recorded_one(data, typed):
    assert GOLDEN_TYPED["block_size"] == cases.BS and GOLDEN_TYPED["fields"] == GOLDEN["fields"]
    assert len(typed) == 14 * cases.BS + 10                             # fourteen whole blocks and a copy block
    assert typed[:9 * cases.BS] == data[:9 * cases.BS]
    assert NEW == ["EXE", "TEXT", "DNA"] and cases.T_TYPED[:14] == cases.T


@pytest.mark.parametrize("ps", cases.PASSES)
def test_typed_table_leaves_nothing_out(ps):
    """All 93 pairs with a new stage in either position are recorded; in pass B each new stage meets all eight coders in first and in
    second position, and the pass holds every checksum width and job count."""
    assert cases.MAX_LEFT_OUT_TYPED == 0
    recs = cases.records_typed(GOLDEN_TYPED, ps)
    assert sorted(recs) == sorted((i, j) for i in range(17) for j in range(17) if i >= 14 or j >= 14) and len(recs) == 17 * 17 - 14 * 14
    assert [r["chain"] for r in recs.values() if "left_out" in r] == []
    assert all(r["chain"] == cases.T_TYPED[i] + "+" + cases.T_TYPED[j] for (i, j), r in recs.items())
    if ps == "A":
        assert {(r["entropy"], r["checksum"], r["jobs"]) for r in recs.values()} == {("NONE", 0, 1)}
    else:
        for pos in (0, 1):
            met = {(r["chain"].split("+")[pos], r["entropy"]) for r in recs.values()}
            assert met >= {(t, e) for t in NEW for e in cases.E}, pos
        assert {r["checksum"] for r in recs.values()} == {0, 32, 64} and {r["jobs"] for r in recs.values()} == {1, 2, 3}
    refused = sorted(r["chain"] for (i, j), r in recs.items() if cases.refused_when_encoding(i, j, cases.T_TYPED, cases.SETS_TYPE_TYPED))
    assert refused == sorted(a + "+" + b for a in NEW for b in ("LZ", "LZX"))


@pytest.mark.parametrize("ps", cases.PASSES)
def test_typed_recorded_digests_are_the_references(ref, typed, ps):
    n = 0
    for r in cases.records_typed(GOLDEN_TYPED, ps).values():
        rc, knz = ref.compress(typed, r["chain"], r["entropy"], cases.BS, jobs=r["jobs"], checksum=r["checksum"], orig_size=len(typed))
        assert rc == 0, r
        assert (len(knz), md5(knz)) == (r["knz_len"], r["knz_md5"]), r
        n += 1
    assert n == 93


@pytest.mark.parametrize("stage", NEW)
def test_every_typed_stage_accepts_and_refuses(ref, typed, stage):
    """Alone on the fourteen whole blocks: EXE takes the x86, the ARM64 and the ELF block, TEXT the three of text, DNA the two of four
    symbols, and each refuses the rest."""
    taken = []
    for b in range(14):
        blk = typed[b * cases.BS:(b + 1) * cases.BS]
        ok, _, skip = ref.forward(stage, blk, len(blk) + 2048)
        assert ok in (0, 1) and bool(skip & 0x80) == (ok == 0), (stage, b, ok, skip)
        if ok:
            taken.append(b)
    assert 1 <= len(taken) <= 13, (stage, taken)
    assert taken == {"EXE": [9, 10, 12], "TEXT": [0, 8, 13], "DNA": [2, 11]}[stage]


@pytest.mark.parametrize("stage", cases.MAY_REFUSE_TYPED)
def test_refusing_stages_do_both_on_the_typed_input(ref, typed, stage):
    taken = sum(ref.forward(stage, typed[b * cases.BS:(b + 1) * cases.BS], cases.BS + 2048)[0] for b in range(14))
    assert 1 <= taken <= 13, (stage, taken)
