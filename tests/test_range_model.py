"""tests/range_model.py -- the Python restatement of the RANGE coder the other RANGE tests lean on -- against the reference's streams
recorded in tests/golden/range.json (tools/make_range_golden.py), and its decoder against its encoder."""
import hashlib
import importlib
import json
import os

import pytest

import knzlib
import range_cases
import range_model

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "range.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def model_stream(rec, data):
    knzlib.load_pkg()
    framing = importlib.import_module("kanzi_amd.framing")
    hdr, bits = framing.make_header(4, 0, rec["block_size"], rec["checksum"], rec["orig_size"])
    assert bits == rec["header_bits"]
    hasher = None
    if rec["checksum"]:
        o = knzlib.Oracle()
        fn = o.L.knzo_xxhash32 if rec["checksum"] == 32 else o.L.knzo_xxhash64
        hasher = lambda b: fn(knzlib._buf(b), len(b), 0x4B414E5A)  # noqa: E731
    return range_model.stream(hdr, bits, data, rec["block_size"], rec["checksum"], hasher)


@pytest.mark.parametrize("rec", GOLDEN["streams"], ids=lambda r: r["name"])
def test_model_writes_the_reference_stream(rec):
    """Every log range from 8 to 12, groups of 6 and of 8, one-symbol and full alphabets, n == scale, chunks without payload, the
    underflow branch, copy blocks, several blocks with 32- and 64-bit checksums: byte for byte what the reference's CLI wrote."""
    data = range_cases.make(rec["recipe"])
    assert md5(data) == rec["input_md5"]
    enc = model_stream(rec, data)
    assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]


@pytest.mark.parametrize("rec", GOLDEN["streams"], ids=lambda r: r["name"])
def test_model_decoder_inverts_its_encoder(rec):
    data = range_cases.make(rec["recipe"])[:rec["block_size"]]
    enc, bits = range_model.encode(data)
    back, used = range_model.decode(enc, len(data), 0, bits)
    assert back == data and used == bits
    # the same bits behind 5 others: nothing in the coder is byte aligned
    shifted = (((0x1F << (8 * len(enc))) | int.from_bytes(enc, "big")) << 3).to_bytes(len(enc) + 1, "big")
    back, used = range_model.decode(shifted, len(data), 5, 5 + bits)
    assert back == data and used == bits


def test_underflow_case_takes_the_underflow_branch():
    st = range_model.Stats()
    range_model.encode(range_cases.make(range_cases.UNDERFLOW), st)
    assert st.underflows >= 1


def test_units_stay_below_the_derived_bound():
    """Every unit raises log2(range) by more than 12 and a byte lowers it by at most 12.1, so a chunk of n bytes leaves at most
    n + n / 64 + 2 units; no byte leaves more than two."""
    for _, r, bs, _ in range_cases.STREAMS:
        data = range_cases.make(r)[:bs]
        st = range_model.Stats()
        range_model.encode(data, st)
        for i, u in enumerate(st.units):
            assert u <= 32768 + 32768 // 64 + 2
