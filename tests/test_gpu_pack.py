"""PACK (AliasCodec, transform id 18) on the device: per stage through the C ABI (with and without a Context data type), in whole
chains through knz_hip_encode_blocks on a batch whose blocks have different data types, and in .knz files whose TEXT / UTF stages
run on the host. Expected results come from tests/golden/pack.json (written from the reference by
tools/make_pack_golden.py)."""
import hashlib
import importlib
import json
import os

import pytest

import pack_cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def _input(rec):
    d = pack_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["recipe"]
    return d


def test_stage_forward_golden_and_round_trip(hip):
    """Every forward path: one symbol, 2-bit and 4-bit packing at lengths 1, 2 and 3 mod 4, digram aliasing with an odd tail and with
    the phantom pair (0, src[0]), and the refusals (below 1024 bytes, fewer than 16 absent values, low savings)."""
    for rec in GOLDEN["stage"]:
        d = _input(rec)
        ok, fwd = hip.transform_forward("PACK", d, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec["recipe"])
        if not rec["ok"]:
            continue
        assert len(fwd) == rec["fwd_len"] and md5(fwd) == rec["fwd_md5"], ("forward", rec["recipe"])
        if "fwd_hex" in rec:
            assert fwd.hex() == rec["fwd_hex"]
        ok, back = hip.transform_inverse("PACK", fwd, len(d))
        assert ok and back == d, ("round trip", rec["recipe"])


def test_stage_refuses_short_destination(hip):
    d = pack_cases.make(["text", 100001, 8])
    ok, _ = hip.transform_forward("PACK", d, len(d) + 1023)
    assert not ok


def test_stage_inverse_of_arbitrary_bytes(hip):
    """Random, truncated and header-shaped inputs at three capacities: the same ok flag and bytes as the reference's inverse."""
    for rec in GOLDEN["inverse"]:
        d = _input(rec)
        ok, inv = hip.transform_inverse("PACK", d, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec["recipe"], rec["cap"])
        if rec["ok"]:
            assert md5(inv) == rec["inv_md5"], ("inverse", rec["recipe"], rec["cap"])


@pytest.mark.parametrize("idx", range(len(pack_cases.STREAM_CHAINS)))
def test_chain_with_mixed_data_types_bit_exact(hip, idx):
    """One batch of text, WAV, BMP, random, DNA-like and 12-symbol blocks, blocks with a RIFF / BMP / PGM / ELF / PNG magic in front
    of a payload PACK would pack (the data type preset makes it refuse), and a 10-byte last block: the stream equals the reference's
    and decodes back. Behind PACK, RLT refuses the DNA block."""
    rec = GOLDEN["streams"][idx]
    data = pack_cases.make(pack_cases.STREAM)
    assert md5(data) == rec["input_md5"]
    bs = rec["block_size"]
    p = hip.params(rec["chain"], rec["entropy"], bs)
    cap = hip.encode_bound(p, len(data))
    d_in, d_out = hip.malloc(len(data) + 64), hip.malloc(cap)
    try:
        hip.h2d(d_in, data)
        bits = hip.encode_blocks(p, d_in, len(data), d_out, cap)
        enc = hip.d2h(d_out, (bits + 7) // 8)
        assert len(enc) == rec["stream_len"] and md5(enc) == rec["stream_md5"], rec["chain"]
        d_dec = hip.malloc(len(data) + bs + 64)
        try:
            ob, _, _ = hip.decode_blocks(p, d_out, bits, 0, d_dec, len(data) + bs)
            assert hip.d2h(d_dec, ob) == data
        finally:
            hip.free(d_dec)
    finally:
        hip.free(d_in)
        hip.free(d_out)


def test_stage_inverse_of_truncated_forward_output(hip):
    """The reference's own PACK outputs cut short: the same ok flag and bytes as its inverse."""
    for rec in GOLDEN["truncated"]:
        d = pack_cases.make(rec["recipe"])
        ok, fwd = hip.transform_forward("PACK", d, len(d) + 1024)
        assert ok
        cut = fwd[:rec["cut"]]
        assert md5(cut) == rec["input_md5"]
        ok, inv = hip.transform_inverse("PACK", cut, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec["recipe"], rec["cut"], rec["cap"])
        if rec["ok"]:
            assert md5(inv) == rec["inv_md5"], ("inverse", rec["recipe"], rec["cut"], rec["cap"])


def test_stage_data_type_in_and_out(hip):
    """knz_hip_transform_forward_dt: PACK refuses MULTIMEDIA, UTF8, EXE and BIN blocks (AliasCodec.cpp:46-55) and leaves the type
    as it was; on an UNDEFINED block it writes detectSimpleType's result (DNA here) and the bytes of a fresh Context; a TEXT block
    keeps TEXT. RLT refuses DNA, BASE64 and UTF8 (RLT.cpp:60-65)."""
    dna = pack_cases.make(["alpha", 8192, 4, 4])
    ok0, ref_bytes = hip.transform_forward("PACK", dna, len(dna) + 1024)
    assert ok0
    for dt in (2, 3, 7, 8):
        ok, _, out = hip.transform_forward_dt("PACK", dna, len(dna) + 1024, dt)
        assert not ok and out == dt, dt
    ok, got, out = hip.transform_forward_dt("PACK", dna, len(dna) + 1024, 0)
    assert ok and got == ref_bytes and out == 6
    ok, got, out = hip.transform_forward_dt("PACK", dna, len(dna) + 1024, 1)
    assert ok and got == ref_bytes and out == 1
    runs = bytes(4096) + b"ab" * 2048
    ok, _ = hip.transform_forward("RLT", runs, len(runs))
    assert ok
    for dt in (5, 6, 8):
        ok, _, out = hip.transform_forward_dt("RLT", runs, len(runs), dt)
        assert not ok and out == dt, dt
    ok, _, _ = hip.transform_forward_dt("RLT", runs, len(runs), 1)
    assert ok


def test_lz_behind_pack_is_refused(hip):
    """The device LZ stages do not take PACK's data type yet (min match 6 for DNA): such chains fail instead of differing."""
    data = pack_cases.make(["text", 1 << 16, 3])
    for chain in ("PACK+LZX", "PACK+LZ", "PACK+ZRLT+LZ"):
        p = hip.params(chain, "HUFFMAN", 1 << 16)
        d_in, d_out = hip.malloc(len(data) + 64), hip.malloc(1 << 20)
        try:
            hip.h2d(d_in, data)
            with pytest.raises(Exception):
                hip.encode_blocks(p, d_in, len(data), d_out, 1 << 20)
        finally:
            hip.free(d_in)
            hip.free(d_out)


@pytest.mark.parametrize("idx", range(len(pack_cases.HOSTED)))
def test_hosted_chain_bit_exact_and_decodes(tmp_path, idx):
    """TEXT / UTF on the host in front of PACK (and RLT) on the device: the data type the host stages leave reaches the device, and
    the .knz equals the reference's and decodes back."""
    import knzlib
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    rec = GOLDEN["hosted"][idx]
    data = pack_cases.make(rec["recipe"])
    assert md5(data) == rec["input_md5"]
    bs = rec["block_size"]
    path = str(tmp_path / "s.knz")
    c = kz.Compressor(path, rec["chain"], rec["entropy"], bs, 1, checksum=rec["checksum"])
    for off in range(0, len(data), bs):
        c.compress(data[off:off + bs])
    c.close()
    enc = open(path, "rb").read()
    assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"], rec["chain"]
    d = kz.Decompressor(path, buffer_size=bs, jobs=1)
    out = bytearray()
    while True:
        chunk = d.decompress(bs)
        out += chunk
        if len(chunk) < bs:
            break
    d.close()
    assert bytes(out) == data
