"""tests/cm_model.py -- the Python restatement of the CM coder the other CM tests lean on -- against the reference's streams recorded
in tests/golden/cm.json (tools/make_cm_golden.py), and its decoder against its encoder. The records with a transform chain in front
of the coder are not restated here (the model has no transforms): the GPU tests compare those with the reference directly."""
import hashlib
import importlib
import json
import os

import pytest

import cm_cases
import cm_model
import knzlib

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cm.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def model_stream(rec, data):
    knzlib.load_pkg()
    framing = importlib.import_module("kanzi_amd.framing")
    hdr, bits = framing.make_header(6, 0, rec["block_size"], rec["checksum"], rec["orig_size"])
    assert bits == rec["header_bits"]
    hasher = None
    if rec["checksum"]:
        o = knzlib.Oracle()
        fn = o.L.knzo_xxhash32 if rec["checksum"] == 32 else o.L.knzo_xxhash64
        hasher = lambda b: fn(knzlib._buf(b), len(b), 0x4B414E5A)  # noqa: E731
    return cm_model.stream(hdr, bits, data, rec["block_size"], rec["checksum"], hasher)


@pytest.mark.parametrize("rec", GOLDEN["streams"], ids=lambda r: r["name"])
def test_model_writes_the_reference_stream(rec):
    """Copy blocks, lengths around 64, var-ints of one to three bytes, constant blocks, pairs and doubled bytes (runMask off and on),
    every row, random bytes, text, the adversary, ragged multi-block inputs with 32- and 64-bit checksums: byte for byte what the
    reference's CLI wrote. These are the records of cm.json whose chain is NONE. The model has no transforms, so the `chains` and
    `hosted` records are not restated here: tests/test_gpu_cm.py compares the device's streams for them with the reference's digests."""
    data = cm_cases.make(rec["recipe"])
    assert md5(data) == rec["input_md5"]
    enc = model_stream(rec, data)
    assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]


@pytest.mark.parametrize("rec", GOLDEN["streams"], ids=lambda r: r["name"])
@pytest.mark.parametrize("big", [cm_model.BIG, 1024])
def test_model_decoder_inverts_its_encoder(rec, big):
    """With the format's chunk rule (one chunk at these sizes) and with the threshold lowered to 1024 bytes (8, 9, 16 or 17 chunks)."""
    data = cm_cases.make(rec["recipe"])[:rec["block_size"]]
    enc, bits = cm_model.encode(data, big)
    back, used = cm_model.decode(enc, len(data), 0, bits, big)
    assert back == data and used == bits
    # the same bits behind 5 others: nothing in the coder is byte aligned
    shifted = (((0x1F << (8 * len(enc))) | int.from_bytes(enc, "big")) << 3).to_bytes(len(enc) + 1, "big")
    back, used = cm_model.decode(shifted, len(data), 5, 5 + bits, big)
    assert back == data and used == bits


def test_chunk_rule():
    """max(count, 64) below the threshold; count >> 3, or count >> 4 when count / 8 reaches the threshold itself."""
    assert cm_model.chunk_len(1) == 64 and cm_model.chunk_len((1 << 26) - 1) == (1 << 26) - 1
    assert cm_model.chunk_len(1 << 26) == 1 << 23 and cm_model.chunk_len((1 << 29) - 1) == ((1 << 29) - 1) >> 3
    assert cm_model.chunk_len(1 << 29) == 1 << 25
    for n, chunks in ((1024, 8), (1031, 9), (8192, 16), (8207, 17)):
        length = cm_model.chunk_len(n, 1024)
        assert -(-n // length) == chunks


def test_varint_cases_have_the_sizes_they_are_named_for():
    want = [(0, 128), (128, 16384), (16384, 1 << 21)]
    for r, (lo, hi) in zip(cm_cases.VARINT, want):
        sizes = []
        cm_model.encode(cm_cases.make(r), payloads=sizes)
        assert len(sizes) == 1 and lo <= sizes[0] < hi, (r, sizes)


def test_adversary_fixture():
    """The fixture says whether the adversary block's payload exceeds the encoder's first staging of n + n / 8 bytes. It does not
    (8,424 bytes for 8,192): no GPU test reaches the second pass with real data, the emulator test (test_emu_cm.py) covers it."""
    a = GOLDEN["adversary"]
    sizes = []
    cm_model.encode(cm_cases.make(cm_cases.ADVERSARY), payloads=sizes)
    assert sizes == [a["payload_bytes"]] and a["first_staging"] == a["n"] + a["n"] // 8
    assert a["exceeds_first_staging"] == (a["payload_bytes"] > a["first_staging"])
    assert a["exceeds_first_staging"] is False
