"""MM (FSDCodec, transform id 15) on the device: per stage through the C ABI (with and without a Context data type), in whole chains
through knz_hip_encode_blocks on a batch whose blocks take every way through the stage, and in a .knz file whose TEXT / UTF stages run
on the host. Expected results come from tests/golden/mm.json (written from the reference by tools/make_mm_golden.py)."""
import hashlib
import importlib
import json
import os

import pytest

import mm_cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mm.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def _input(rec):
    d = mm_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["recipe"]
    return d


def test_stage_forward_golden_and_round_trip(hip):
    """XOR mode (WAV, walks with many jumps, random bytes) and delta mode at distances 1, 2, 3, 4, 8 and 16 with escapes, lengths around
    the tile size and not divisible by 10, 1,024 bytes accepted and 1,023 refused, a block of 1.7 MB (more than 256 tiles and stretches), the overflow blocks, blocks that
    fail only the final check, and the refusals by entropy
    and by magic."""
    for rec in GOLDEN["stage"]:
        d = _input(rec)
        ok, fwd = hip.transform_forward("MM", d, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec["recipe"])
        if not rec["ok"]:
            continue
        assert len(fwd) == rec["fwd_len"] and md5(fwd) == rec["fwd_md5"], ("forward", rec["recipe"])
        assert fwd[0] == rec["mode"] and fwd[1] == rec["dist"]
        ok, back = hip.transform_inverse("MM", fwd, rec["cap"])
        assert ok and back == d, ("round trip", rec["recipe"])


def test_stage_refuses_short_destination(hip):
    """FSDCodec.cpp:117: a destination one byte below getMaxEncodedLength is refused, the bound itself is enough."""
    d = mm_cases.make(["walk", 100003, 65, 16, 0.015])
    ok, _ = hip.transform_forward("MM", d, mm_cases.max_encoded(len(d)) - 1)
    assert not ok
    ok, _ = hip.transform_forward("MM", d, mm_cases.max_encoded(len(d)))
    assert ok


def test_stage_inverse_of_arbitrary_bytes(hip):
    """Random and header-shaped inputs (every guard, each distance in both modes, runs of 255 of odd and even length, an escape as the
    last byte, all-escape payloads) at two capacities: the same ok flag and bytes as the reference's inverse."""
    n_ok = 0
    for rec in GOLDEN["inverse"]:
        d = _input(rec)
        ok, inv = hip.transform_inverse("MM", d, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec["recipe"], rec["cap"])
        if rec["ok"]:
            n_ok += 1
            assert md5(inv) == rec["inv_md5"], ("inverse", rec["recipe"], rec["cap"])
    assert 2 * n_ok >= len(GOLDEN["inverse"])


def test_stage_inverse_of_truncated_forward_output(hip):
    """The reference's own MM outputs cut short: the same ok flag and bytes as its inverse."""
    for rec in GOLDEN["truncated"]:
        d = mm_cases.make(rec["recipe"])
        ok, fwd = hip.transform_forward("MM", d, mm_cases.max_encoded(len(d)))
        assert ok
        cut = fwd[:rec["cut"]]
        assert md5(cut) == rec["input_md5"]
        ok, inv = hip.transform_inverse("MM", cut, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec["recipe"], rec["cut"], rec["cap"])
        if rec["ok"]:
            assert md5(inv) == rec["inv_md5"], ("inverse", rec["recipe"], rec["cut"], rec["cap"])


def test_stage_data_type_in_and_out(hip):
    """knz_hip_transform_forward_dt: MM looks only at UNDEFINED, MULTIMEDIA and BIN blocks (FSDCodec.cpp:124-129) and leaves the others
    as they were; success leaves MULTIMEDIA; so do the overflow and a failed final check (:206, :270, :285); the quick exit writes detectSimpleType's verdict of the
    samples over whatever was there (:198-204: DNA for a block of ACGT, UNDEFINED for text); a refusing magic leaves the type."""
    w = mm_cases.make(["walk", 100003, 65, 16, 0.015])
    cap = mm_cases.max_encoded(len(w))
    ok0, ref_bytes = hip.transform_forward("MM", w, cap)
    assert ok0
    for dt in (1, 3, 4, 5, 6, 8, 9):
        ok, _, out = hip.transform_forward_dt("MM", w, cap, dt)
        assert not ok and out == dt, dt
    for dt in (0, 2, 7):
        ok, got, out = hip.transform_forward_dt("MM", w, cap, dt)
        assert ok and got == ref_bytes and out == 2, dt
    over = mm_cases.make(["overflow", 200000, 74, 1])
    ok, _, out = hip.transform_forward_dt("MM", over, mm_cases.max_encoded(len(over)), 7)
    assert not ok and out == 2
    final = mm_cases.make(["finalfail", 200000, 82])
    ok, _, out = hip.transform_forward_dt("MM", final, mm_cases.max_encoded(len(final)), 0)
    assert not ok and out == 2
    dna = mm_cases.make(["alpha", 50000, 77, 4])
    for dt in (0, 2, 7):
        ok, _, out = hip.transform_forward_dt("MM", dna, mm_cases.max_encoded(len(dna)), dt)
        assert not ok and out == 6, dt
    text = mm_cases.make(["text", 100000, 76])
    ok, _, out = hip.transform_forward_dt("MM", text, mm_cases.max_encoded(len(text)), 2)
    assert not ok and out == 0
    png = mm_cases.make(["magic", 100000, 0, "89504e47", ["walk", 100000, 79, 1, 0.01]])
    ok, _, out = hip.transform_forward_dt("MM", png, mm_cases.max_encoded(len(png)), 7)
    assert not ok and out == 7
    short = mm_cases.make(["walk", 1023, 72, 1, 0.01])
    ok, _, out = hip.transform_forward_dt("MM", short, mm_cases.max_encoded(len(short)), 2)
    assert not ok and out == 2


@pytest.mark.parametrize("idx", range(len(mm_cases.STREAM_CHAINS)))
def test_chain_bit_exact_and_decodes(hip, idx):
    """One batch of WAV, walks, text, a DNA-like block, the overflow block, blocks with a PNG and a PGM magic in front of a walk and a
    5,000-byte tail: the stream equals the reference's and decodes back (decode ranges on). RLT and PACK behind MM see the data
    type MM leaves."""
    rec = GOLDEN["streams"][idx]
    data = mm_cases.make(mm_cases.STREAM)
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


def test_lz_behind_mm_is_refused(hip):
    """MM sets the data type, which the device LZ stages do not read yet: such chains fail instead of differing, with the
    message of the refusal behind PACK."""
    data = mm_cases.make(["walk", 1 << 16, 160, 1, 0.01])
    for chain in ("MM+LZX", "MM+LZ", "PACK+MM+LZX"):
        p = hip.params(chain, "HUFFMAN", 1 << 16)
        d_in, d_out = hip.malloc(len(data) + 64), hip.malloc(1 << 20)
        try:
            hip.h2d(d_in, data)
            with pytest.raises(Exception, match="LZ / LZX behind PACK is not implemented on device"):
                hip.encode_blocks(p, d_in, len(data), d_out, 1 << 20)
        finally:
            hip.free(d_in)
            hip.free(d_out)


@pytest.mark.parametrize("idx", range(len(mm_cases.HOSTED)))
def test_hosted_chain_bit_exact_and_decodes(tmp_path, idx):
    """TEXT / UTF on the host in front of PACK and MM on the device: the .knz equals the reference's and decodes back."""
    import knzlib
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    rec = GOLDEN["hosted"][idx]
    data = mm_cases.make(rec["recipe"])
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
