"""BWTS (bijective BWT, transform id 2) on the device: per stage through the C ABI, whole streams through the C API / host mirror,
block-range and sharded decoding, one large block. Expected bytes come from tests/golden/bwts.json (written from the reference by
tools/make_bwts_golden.py); where the reference build (oracle/_ref) is present, test_against_reference_build checks it directly too."""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import bwts_cases
import knzlib

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bwts.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def _kanzi():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.kanzi")


def _input(rec):
    d = bwts_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["recipe"]
    return d


def test_stage_forward_and_inverse_golden(hip):
    """Forward output equal to the reference's (fixture), inverse gives the input back, and the inverse of the raw bytes (every
    byte string is a BWTS output) equal to the reference's inverse: sizes 0, 1, 2, mississippi, the pi digits, SIX.MIXED...,
    all bytes equal, strictly decreasing, abab..., a^k b, random, text, zero runs."""
    for rec in GOLDEN["stage"]:
        d = _input(rec)
        ok, fwd = hip.transform_forward("BWTS", d, len(d))
        assert ok and len(fwd) == len(d), rec["recipe"]
        if rec["kind"] == "stage":
            assert md5(fwd) == rec["fwd_md5"], ("forward", rec["recipe"])
            if "fwd_hex" in rec:
                assert fwd.hex() == rec["fwd_hex"]
        ok, back = hip.transform_inverse("BWTS", fwd, len(d))
        assert ok and back == d, ("round trip", rec["recipe"])
        ok, inv = hip.transform_inverse("BWTS", d, len(d))
        assert ok and md5(inv) == rec["inv_md5"], ("inverse of raw bytes", rec["recipe"])


def test_stage_refuses_short_destination(hip):
    d = b"mississippi"
    ok, _ = hip.transform_forward("BWTS", d, len(d) - 1)
    assert not ok
    ok, _ = hip.transform_inverse("BWTS", d, len(d) - 1)
    assert not ok


def _compress(kz, path, data, chain, entropy, bs, ck):
    c = kz.Compressor(path, chain, entropy, bs, 1, checksum=ck)
    for off in range(0, len(data), bs):
        c.compress(data[off:off + bs])
    c.close()
    return open(path, "rb").read()


def _decompress(kz, path, bs):
    d = kz.Decompressor(path, buffer_size=bs, jobs=1)
    out = bytearray()
    while True:
        chunk = d.decompress(bs)
        out += chunk
        if len(chunk) < bs:
            break
    d.close()
    return bytes(out)


@pytest.mark.parametrize("idx", range(len(GOLDEN["streams"])))
def test_stream_bit_exact_and_decodes(tmp_path, idx):
    """The whole stream (C API, host mirror; TEXT and UTF on the host in front of BWTS) byte-identical to the reference's .knz
    (fixture md5), so the reference's own stream is what is decoded back."""
    rec = GOLDEN["streams"][idx]
    kz = _kanzi()
    data = _input(rec)
    path = str(tmp_path / "s.knz")
    enc = _compress(kz, path, data, rec["chain"], rec["entropy"], rec["block_size"], rec["checksum"])
    assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"], (rec["chain"], rec["entropy"])
    assert _decompress(kz, path, rec["block_size"]) == data


def _header_bits(hip, rec):
    fr = importlib.import_module("kanzi_amd.framing")
    p = hip.params(rec["chain"], rec["entropy"], rec["block_size"], rec["checksum"])
    return p, fr.make_header(p.entropy_type, p.transform_type, rec["block_size"], rec["checksum"], rec["n"])


def test_decode_in_block_ranges_and_sharded(hip):
    """encode_blocks (C ABI) byte-identical to the reference stream; decode_blocks over ranges of 1, 3 and 4 blocks, and the sharded
    decode path over 3 ranks, give the bytes of a whole-stream decode."""
    rec = GOLDEN["ranged"]
    data = _input(rec)
    bs, n = rec["block_size"], rec["n"]
    p, (hdr, hb) = _header_bits(hip, rec)
    cap = hip.encode_bound(p, n) + 64
    d_in, d_out = hip.malloc(n + 64), hip.malloc(cap)
    hip.h2d(d_in, data)
    bits = hip.encode_blocks(p, d_in, n, d_out, cap, prologue=hdr, prologue_bits=hb)
    enc = hip.d2h(d_out, (bits + 7) // 8)
    hip.free(d_in)
    assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]
    d_dec = hip.malloc(n + bs + 64)
    ob, _, nb = hip.decode_blocks(p, d_out, bits, hb, d_dec, n + bs)
    whole = hip.d2h(d_dec, ob)
    assert whole == data and nb == (n + bs - 1) // bs
    out, start, done = bytearray(), hb, 0
    for step in (1, 3, 4, 100):
        ob, start, k = hip.decode_blocks(p, d_out, bits, start, d_dec, n + bs, max_blocks=step)
        out += hip.d2h(d_dec, ob)
        done += k
        if done == nb:
            break
    assert bytes(out) == whole
    hip.free(d_out); hip.free(d_dec)
    sh = importlib.import_module("kanzi_amd.sharded")
    dec = sh.DeviceRunDecoder(0)
    parts = [None] * 3
    for r in range(3):
        def gather(obj, r=r):
            parts[r] = obj
            return None
        sh.decompress_sharded(enc, r, 3, dec, gather)
    assert b"".join(parts) == whole


def test_big_single_block(hip):
    """One 256 MiB block: forward digest equal to the reference's (fixture), inverse gives it back."""
    rec = GOLDEN["big"]
    data = _input(rec)
    ok, fwd = hip.transform_forward("BWTS", data, len(data))
    assert ok and md5(fwd) == rec["fwd_md5"]
    ok, back = hip.transform_inverse("BWTS", fwd, len(data))
    assert ok and back == data


def test_against_reference_build(hip, ref):
    """Source: the reference build in oracle/_ref (skipped where it is absent). Fresh random inputs: forward and inverse of the raw
    bytes equal to the reference's."""
    rng = np.random.default_rng(2024)
    for k in range(12):
        n = int(rng.integers(2, 40000))
        alpha = int(rng.choice([2, 3, 4, 256]))
        d = rng.integers(0, alpha, n, dtype=np.uint8).tobytes()
        ok, want, _ = ref.forward("BWTS", d, len(d))
        got_ok, got = hip.transform_forward("BWTS", d, len(d))
        assert ok and got_ok and got == want, (k, n, alpha)
        ok, want = ref.inverse("BWTS", d, len(d))
        got_ok, got = hip.transform_inverse("BWTS", d, len(d))
        assert ok and got_ok and got == want, (k, n, alpha)
