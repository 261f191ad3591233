"""tests/tpaq_model.py -- the Python restatement of the TPAQ / TPAQX coders the other TPAQ tests lean on -- against the reference's
streams recorded in tests/golden/tpaq.json (tools/make_tpaq_golden.py), its decoder against its encoder, and the sizing of the
predictor (the model's and the library's own, through the C ABI) against a table written out from the reference's constructor.
The records with a transform chain in front of the coder are not restated here (the model has no transforms): the GPU tests compare
those with the reference directly."""
import hashlib
import importlib
import json
import os

import pytest

import knzlib
import tpaq_cases
import tpaq_model

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tpaq.json")))
MIB = 1 << 20


def md5(b):
    return hashlib.md5(b).hexdigest()


def model_stream(rec, data):
    knzlib.load_pkg()
    framing = importlib.import_module("kanzi_amd.framing")
    hdr, bits = framing.make_header(tpaq_cases.ENTROPY_ID[rec["coder"]], 0, rec["block_size"], rec["checksum"], rec["orig_size"])
    assert bits == rec["header_bits"] and hdr.hex() == rec["header_hex"]
    hasher = None
    if rec["checksum"]:
        o = knzlib.Oracle()
        fn = o.L.knzo_xxhash32 if rec["checksum"] == 32 else o.L.knzo_xxhash64
        hasher = lambda b: fn(knzlib._buf(b), len(b), 0x4B414E5A)  # noqa: E731
    return tpaq_model.stream(hdr, bits, data, tpaq_cases.EXTRA[rec["coder"]], rec["block_size"], rec["checksum"], hasher)


@pytest.mark.parametrize("rec", GOLDEN["streams"], ids=lambda r: "%s-%s" % (r["name"], r["coder"]))
def test_model_writes_the_reference_stream(rec):
    """Copy blocks and the first coded lengths, constant bytes, every byte value, random bytes, pairs, text with long repeats (the match
    model starts, reaches 88, is cleared by a mispredicted bit), mostly binary input, input that crosses _binCount against pos >> 3
    and pos >> 2 in both directions, every tier of the states table (block sizes 1024, 4096, 1, 4, 16 and 64 MiB), masks that are not
    2^k - 1 (block size 10000: the reference reads these streams back itself, the generator checks), ragged multi-block inputs with
    32- and 64-bit checksums: byte for byte what the reference's CLI wrote, for TPAQ and TPAQX."""
    data = tpaq_cases.make(rec["recipe"])
    assert md5(data) == rec["input_md5"]
    enc = model_stream(rec, data)
    assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]


INVERT = [r for r in GOLDEN["streams"] if r["name"] in ("len16", "len65", "len4097", "const", "random", "binary", "bs10000", "bs64m")]


@pytest.mark.parametrize("rec", INVERT, ids=lambda r: "%s-%s" % (r["name"], r["coder"]))
def test_model_decoder_inverts_its_encoder(rec):
    """From bit 0 and behind 5 other bits (nothing in the coder is byte aligned); with the format's chunk rule and, for the short
    records, with the threshold lowered to 1,024 bytes (8 chunks and more). With a states table of 2^10 bytes as well."""
    data = tpaq_cases.make(rec["recipe"])[:rec["block_size"]]
    x, bs = tpaq_cases.EXTRA[rec["coder"]], rec["block_size"]
    variants = [(tpaq_model.BIG, None)] + ([(1024, None), (tpaq_model.BIG, 10)] if len(data) <= 4097 else [])
    for big, sl in variants:
        enc, bits = tpaq_model.encode(data, x, bs, big, states_log=sl)
        shifted = (((0x1F << (8 * len(enc))) | int.from_bytes(enc, "big")) << 3).to_bytes(len(enc) + 1, "big")
        back, used = tpaq_model.decode(shifted, len(data), x, bs, 5, 5 + bits, big, states_log=sl)
        assert back == data and used == bits
        if big == tpaq_model.BIG and sl is None and len(data) <= 4097:
            back, used = tpaq_model.decode(enc, len(data), x, bs, 0, bits, big)
            assert back == data and used == bits


# TPAQPredictor.hpp:312-358 written out: (from this block size, states bytes), (from this block length, mixers)
STATES = [(0, 4 * MIB), (MIB, 16 * MIB), (4 * MIB, 64 * MIB), (16 * MIB, 128 * MIB), (64 * MIB, 256 * MIB)]
MIXERS = [(0, 1 << 8), (MIB, 1 << 11), (4 * MIB, 1 << 13), (8 * MIB, 1 << 14), (16 * MIB, 1 << 15), (32 * MIB, 1 << 16)]


def _expected(rbsz, absz, extra):
    states = [v for t, v in STATES if rbsz >= t][-1]
    mixers = [v for t, v in MIXERS if absz >= t][-1]
    hsz = min(16 * MIB, absz * 16)
    return states << (2 * extra), mixers << (2 * extra), hsz << (2 * extra), min(rbsz, 64 * MIB), 256, 65536 if extra else 256


def test_sizes_at_every_threshold_and_one_below():
    """The model's params() and the library's knz_hip_tpaq_params against the table, for TPAQ and TPAQX (all of states, mixers and
    hash << 2): every threshold of the block size and of the block length, one below each, and the ends."""
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    edges_bs = sorted({v for t, _ in STATES[1:] for v in (t - 1, t)} | {1024, 10000, (1 << 30) - 16, 1 << 30})
    edges_len = sorted({v for t, _ in MIXERS[1:] for v in (t - 1, t)} | {16, 10000, MIB - 1, (1 << 26) - 1, 1 << 26})
    for extra in (0, 1):
        for rbsz in edges_bs:
            for absz in edges_len:
                if absz > rbsz + rbsz // 8 + 8192:
                    continue
                want = _expected(rbsz, absz, extra)
                assert tpaq_model.params(rbsz, absz, extra) == want, (rbsz, absz, extra)
                assert hipapi.tpaq_params(rbsz, absz, extra) == want, (rbsz, absz, extra)
    # the examples of the format's description: -b 10000 gives a buffer mask of 9999 and, for a block of 5,000 bytes, a hash mask of 79999
    assert tpaq_model.params(10000, 5000, 0)[2:4] == (80000, 10000)
    assert hipapi.tpaq_params(64 * MIB, 64 * MIB, 1)[:4] == (1 << 30, 1 << 18, 64 * MIB, 64 * MIB)
