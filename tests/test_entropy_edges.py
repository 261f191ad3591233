"""The inputs of tests/entropy_edge_cases.py on the CPU: every case has the property it is named for (derived again from its bytes,
and for Huffman code lengths from the oracle's own chunk headers), the oracle writes what tests/golden/entropy_edges.json records
of the unmodified reference and reads it back, and -- where the reference build is present -- the reference still does the same.
No case is left out or exempted. The same inputs on the kernels: tests/test_emu_entropy_edges.py, tests/test_gpu_entropy_edges.py."""
import hashlib
import json
import os

import pytest

import entropy_edge_cases as eec
from entropy_edge_cases import CH, M4

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entropy_edges.json")


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(FIXTURE))


def md5(b):
    return hashlib.md5(b).hexdigest()


def test_inputs_are_the_fixtures(fixture):
    names = [c[0] for c in eec.stage_cases()] + [b[0] for b in eec.batch_inputs()]
    assert list(fixture["inputs"]) == names
    for name, data, prop in eec.stage_cases():
        assert md5(data) == fixture["inputs"][name], name
    for name, bs, data in eec.batch_inputs():
        assert md5(data) == fixture["inputs"][name], name
    assert set(fixture["stage"]) == {c[0] for c in eec.stage_cases()}
    assert all(set(v) == set(eec.CODERS) for v in fixture["stage"].values())
    assert len(fixture["batch"]) == len(eec.batch_inputs()) * len(eec.CODERS) * len(eec.BATCH_CHECKSUMS)


def test_cases_have_the_properties_they_are_named_for(oracle):
    cases = {name: (data, prop) for name, data, prop in eec.stage_cases()}
    # lengths: every listed length once, every chunk an ordinary coded chunk (more than one symbol wherever it has two bytes)
    assert [len(cases["len:%d" % n][0]) for n in eec.LENGTHS] == list(eec.LENGTHS)
    for n in eec.LENGTHS:
        data, prop = cases["len:%d" % n]
        asz = eec.chunk_alphabets(data)
        assert len(asz) == prop["chunks"] and len(data) - (len(asz) - 1) * CH == prop["last_chunk"], n
        assert all(a > 100 for a in asz[:-1]) and (asz[-1] > 1 or prop["last_chunk"] == 1), n
    assert {cases["len:%d" % n][1]["last_chunk"] for n in eec.LENGTHS} >= {1, 2, 3, 4, 31, 32, 33, 4096, CH - 1, CH}
    assert {cases["len:%d" % n][1]["chunks"] for n in eec.LENGTHS} >= {1, 2, 15, 16, 17, 18, 64, 65}
    # alphabets: exactly k distinct symbols in every chunk, at the named end of the byte range
    seen = set()
    for name, (data, prop) in cases.items():
        if not name.startswith("asz:"):
            continue
        k = prop["asz"]
        assert eec.chunk_alphabets(data) == [k] * ((len(data) + CH - 1) // CH), name
        assert len(data) == prop["len"] and len(data) in (CH + 777, max(k, 33) + 5), name
        if prop["place"] == "low":
            assert max(data) == k - 1, name
        elif prop["place"] == "high":
            assert min(data) == 256 - k, name
        seen.add((k, prop["place"], len(data) > CH))
    assert seen == {(k, p, two) for k in eec.ALPHABET_SIZES for p in (eec.PLACEMENTS if k < 256 else ("low",)) for two in (False, True)}
    # chunk kinds
    data, prop = cases["kinds"]
    assert eec.chunk_alphabets(data) == prop["chunk_asz"] and len(data) == 5 * CH + 100
    assert len({data[0], data[2 * CH], data[5 * CH]}) == 3
    # Huffman: the lengths the oracle wrote into its chunk headers; the optimal ones where the frequencies leave no choice
    for name, (data, prop) in cases.items():
        if not name.startswith("huff:"):
            continue
        enc, bits = oracle.entropy_encode("HUFFMAN", data)
        lens, delta_bits = eec.huffman_chunk_headers(enc, len(data))[prop["chunk"]]
        chunk = data[prop["chunk"] * CH:(prop["chunk"] + 1) * CH]
        assert set(lens) == set(chunk), name
        if "max_code_len" in prop:
            assert max(lens.values()) == prop["max_code_len"], (name, max(lens.values()))
            plain, tie = eec.huffman_lengths({s: chunk.count(s) for s in set(chunk)})
            assert not tie and max(plain.values()) == prop["optimal_len"], (name, tie, max(plain.values()))
            assert (plain == lens) == (prop["optimal_len"] <= 12), name
        if "asz" in prop:
            assert len(lens) == prop["asz"], name
        if "long_codes" in prop:      # codes of 11 and 12 bits: slots of the 512-entry table
            slots = sum(1 << (12 - l) for l in lens.values() if l > 10)
            assert sum(1 for l in lens.values() if l > 10) >= prop["long_codes"] and 448 <= slots <= 512, (name, slots)
            top = sorted(chunk.count(s) for s in set(chunk))[-3:]
            assert top == [2048, 4096, 8192], name
        if "slots_from_10" in prop:   # 12-bit slots of the codes of 10 bits and more, and of the long codes of the chunk behind
            assert sum(1 << (12 - l) for l in lens.values() if l >= 10) == prop["slots_from_10"] > 512, name
            assert sorted(set(lens.values())) == [1, 8, 10, 11], name
            nxt = eec.huffman_chunk_headers(enc, len(data))[prop["chunk"] + 1][0]
            assert sum(1 << (12 - l) for l in nxt.values() if l > 10) >= prop["next_long_slots"], name
        if "delta_bits" in prop:
            ls = [lens[s] for s in range(256)]
            assert all(abs(a - b) >= 3 for a, b in zip(ls, ls[1:])) and delta_bits > prop["delta_bits"], (name, delta_bits)
    # ANS1: context totals as the order-1 histogram counts them
    data, prop = cases["ans1:ctx2048"]
    tot = eec.order1_context_totals(data)
    assert {c: int(tot[c]) for c in prop["ctx_totals"]} == prop["ctx_totals"] and 32 < len(data) <= M4
    data, prop = cases["ans1:sparse"]
    assert int((eec.order1_context_totals(data) > 0).sum()) == prop["contexts"]
    assert [len(cases["m4:%d" % n][0]) for n in eec.M4_CUTS] == list(eec.M4_CUTS)
    assert {cases["m4:%d" % n][1]["last_chunk_ans1"] for n in eec.M4_CUTS} >= {1, 2, 3, 4, 7, 33, M4 - 1, M4}
    # batches: slots per block that do not divide the 16 of a decode wave, a 16-byte second chunk, every tail
    for name, bs, data in eec.batch_inputs():
        assert len(data) // bs == eec.BATCH_BLOCKS and len(data) % bs in eec.BATCH_TAILS
    assert {(bs + CH - 1) // CH for bs in eec.BATCH_BLOCK_SIZES} == {2, 3, 5} and eec.BATCH_BLOCK_SIZES[0] - CH == 16
    kinds = {min(len(set(eec.batch_master()[at:at + CH])), 4) for at in range(0, 10 * CH, CH)}
    assert kinds == {1, 3, 4}


@pytest.mark.parametrize("coder", eec.CODERS)
def test_oracle_writes_the_fixture_and_reads_it_back(oracle, fixture, coder):
    for name, data, prop in eec.stage_cases():
        enc, bits = oracle.entropy_encode(coder, data)
        assert enc is not None, (name, bits)
        assert [bits, len(enc), md5(enc)] == fixture["stage"][name][coder], name
        r, back = oracle.entropy_decode(coder, enc, len(data))
        assert r == len(data) and back == data, (name, r)


@pytest.mark.parametrize("coder", eec.CODERS)
def test_oracle_writes_the_fixture_batches_and_reads_them_back(oracle, fixture, coder):
    for name, bs, data in eec.batch_inputs():
        for ck in eec.BATCH_CHECKSUMS:
            rc, enc = oracle.compress(data, "NONE", coder, bs, checksum=ck, headerless=1)
            assert rc == 0 and [len(enc), md5(enc)] == fixture["batch"][eec.batch_key(name, coder, ck)], (name, ck)
            rc, full = oracle.compress(data, "NONE", coder, bs, checksum=ck)
            assert rc == 0
            rc, back = oracle.decompress(full, len(data))
            assert rc == 0 and back == data, (name, ck)


@pytest.mark.parametrize("coder", eec.CODERS)
def test_reference_writes_the_fixture_and_reads_it_back(ref, fixture, coder):
    for name, data, prop in eec.stage_cases():
        enc, bits = ref.entropy_encode(coder, data)
        assert enc is not None, (name, bits)
        assert [bits, len(enc), md5(enc)] == fixture["stage"][name][coder], name
        r, back = ref.entropy_decode(coder, enc, len(data))
        assert r == len(data) and back == data, (name, r)


@pytest.mark.parametrize("coder", eec.CODERS)
def test_reference_writes_the_fixture_batches_and_reads_them_back(ref, oracle, fixture, coder):
    """The reference reads streams with a header only: it reads back the same blocks behind a header, which the oracle's writer of
    that stream confirms are the same blocks (its headered stream is the reference's)."""
    for name, bs, data in eec.batch_inputs():
        for ck in eec.BATCH_CHECKSUMS:
            rc, enc = ref.compress(data, "NONE", coder, bs, jobs=1, checksum=ck, headerless=1)
            assert rc == 0 and [len(enc), md5(enc)] == fixture["batch"][eec.batch_key(name, coder, ck)], (name, ck)
            rc, full = ref.compress(data, "NONE", coder, bs, jobs=1, checksum=ck)
            assert rc == 0 and full == oracle.compress(data, "NONE", coder, bs, checksum=ck)[1], (name, ck)
            rc, back = ref.decompress(full, len(data))
            assert rc == 0 and back == data, (name, ck)
