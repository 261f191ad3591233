"""The inputs of tests/entropy_edge_cases.py on the device: k_ans0_stats / k_ans0_encode, k_ans1_hist / k_ans1_ctx / k_ans1_encode,
k_huff_encode, the FPAQ phases and the bit assembly must write the reference's bits (tests/golden/entropy_edges.json, and byte for
byte the oracle's, which tests/test_entropy_edges.py pins to that fixture); k_ans_scan / k_ans0_decode / k_ans1_decode, k_huff_scan /
k_huff_decode and the FPAQ decoder must read them back, consuming exactly the stream's bits, also from bit offsets 1 and 13 for the
cases whose header windows and fill paths depend on the alignment. The batches put 2, 3 and 5 chunk slots per block in front of
decode waves of 16 slots, with chunks of every kind next to each other.

One test per family and coder: a failure names its case in the assert message."""
import hashlib
import importlib
import json
import os

import pytest

import entropy_edge_cases as eec
from test_gpu_parity import gpu_compress, gpu_decompress

pytestmark = pytest.mark.gpu

# (FPAQ is one serial chain per sub-chunk of 4 MiB: its three 4 MiB cuts are a test each, the other coders' cuts one test together)
FAMILIES = {"len_short": lambda name, n: name.startswith("len:") and n <= eec.EMU_MAX,
            "len_long": lambda name, n: name.startswith("len:") and n > eec.EMU_MAX,
            "asz": lambda name, n: name.startswith("asz:"),
            "structure": lambda name, n: name.startswith(("kinds", "huff:", "ans1:")),
            "m4": lambda name, n: name.startswith("m4:")}
FAMILY_CODERS = [(f, c) for f in FAMILIES for c in eec.CODERS if f != "m4" or c == "ANS1"] + [("m4:%d" % n, "FPAQ") for n in eec.FPAQ_M4_CUTS]


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entropy_edges.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def at_bit_offset(enc, shift):
    """`shift` one-bits in front of the stream."""
    bits = 8 * len(enc) + shift
    pad = (-bits) % 8
    v = (((1 << shift) - 1) << (8 * len(enc))) | int.from_bytes(enc, "big")
    return (v << pad).to_bytes((bits + pad) // 8, "big")


@pytest.mark.parametrize("family,coder", FAMILY_CODERS)
def test_stage_cases(hip, oracle, fixture, family, coder):
    member = FAMILIES.get(family, lambda name, n: name == family)
    n = 0
    for name, data, prop in eec.stage_cases():
        if not member(name, len(data)) or coder not in eec.device_coders(name, data):
            continue
        want, wbits = oracle.entropy_encode(coder, data)
        got, bits = hip.entropy_encode(coder, data)
        assert [bits, len(got), md5(got)] == fixture["stage"][name][coder], (name, bits, len(got))
        assert got == want, name
        dec, out, used = hip.entropy_decode(coder, want, len(data))
        assert dec == len(data) and used == wbits and out == data, (name, dec, used, wbits)
        if eec.offset_case(name, prop):
            for shift in (1, 13):
                dec, out, used = hip.entropy_decode(coder, at_bit_offset(want, shift), len(data), start_bit=shift)
                assert dec == len(data) and used == wbits and out == data, (name, shift, dec, used, wbits)
        n += 1
    assert n >= (3 if family in FAMILIES else 1), n


@pytest.mark.parametrize("coder", eec.CODERS)
@pytest.mark.parametrize("bs", eec.BATCH_BLOCK_SIZES)
def test_batches(hip, oracle, fixture, bs, coder):
    """knz_hip_encode_blocks writes the reference's headerless stream, knz_hip_decode_blocks reads it back: 18 blocks and every tail.
    (dec_parts: a chain without inverse stages stays one range whatever the knob says -- Decoder::plan --, so 1 and 3 must agree.)"""
    L =importlib.import_module("kanzi_amd.hipapi").lib()
    n = 0
    try:
        for name, block, data in eec.batch_inputs():
            if block != bs:
                continue
            for ck in eec.BATCH_CHECKSUMS:
                rc, want = oracle.compress(data, "NONE", coder, bs, checksum=ck, headerless=1)
                assert rc == 0
                out, bits, hb = gpu_compress(hip, data, "NONE", coder, bs, checksum=ck, headerless=1)
                assert [len(out), md5(out)] == fixture["batch"][eec.batch_key(name, coder, ck)], (name, ck, len(out))
                assert out == want, (name, ck)
                # (the block ranges of the decode driver: one range, and up to three, for one block size)
                for parts in ((1, 3) if bs == 3 * eec.CH else (3,)):
                    assert L.knz_hip_tune(b"dec_parts", parts) == 0
                    assert gpu_decompress(hip, want, "NONE", coder, bs, len(data), 0, checksum=ck) == data, (name, ck, parts)
                n += 1
    finally:
        L.knz_hip_tune(b"dec_parts", 3)
    assert n == len(eec.BATCH_TAILS) * len(eec.BATCH_CHECKSUMS)
