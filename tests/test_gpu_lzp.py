"""LZP (LZPCodec, transform id 14) on the device: per stage through the C ABI, in whole chains through knz_hip_encode_blocks /
knz_hip_decode_blocks, in a .knz file with a host stage in front, and through the command-line tool. Expected results come from
tests/golden/lzp.json (written from the reference by tools/make_lzp_golden.py)."""
import hashlib
import importlib
import json
import os
import subprocess

import pytest

import lzp_cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lzp.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def _input(rec):
    d = lzp_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["recipe"]
    return d


@pytest.fixture(scope="module")
def forward_outputs(hip):
    """The device's forward result of every stage record, computed once."""
    out = {}
    for rec in GOLDEN["stage"]:
        d = _input(rec)
        out[json.dumps(rec["recipe"])] = (d, hip.transform_forward("LZP", d, rec["cap"]))
    return out


def test_stage_forward_golden_and_round_trip(hip, forward_outputs):
    """Lengths around every guard and the batch of 64, matches of 63 (refused), 64, 64 + 253, 64 + 254, 64 + 2 * 254 + 1 and 100,000 bytes,
    a match up to the last byte and one inside the last 64, periods 1, 3 and 5, 0xFC with and without escape (tail loop included), matches
    back to back, matches 1 to 3 literals behind a match and through buckets stored 1 to 3 literals behind the block start, positions of
    one batch sharing a bucket, and the three refusals inside the loop."""
    for rec in GOLDEN["stage"]:
        d, (ok, fwd) = forward_outputs[json.dumps(rec["recipe"])]
        if len(d) == 0:
            assert ok and fwd == b""
            continue
        assert int(ok) == rec["ok"], ("ok", rec["recipe"])
        if not rec["ok"]:
            continue
        assert len(fwd) == rec["fwd_len"] and md5(fwd) == rec["fwd_md5"], ("forward", rec["recipe"])
        ok, back = hip.transform_inverse("LZP", fwd, len(d))
        assert ok and back == d, ("round trip", rec["recipe"])


def test_stage_refuses_short_destination(hip):
    """LZCodec.cpp:788: a destination one byte below getMaxEncodedLength is refused, the bound itself is enough."""
    d = lzp_cases.make(lzp_cases.SHORT_CAP)
    ok, _ = hip.transform_forward("LZP", d, lzp_cases.max_encoded(len(d)) - 1)
    assert not ok
    ok, _ = hip.transform_forward("LZP", d, lzp_cases.max_encoded(len(d)))
    assert ok


def test_stage_inverse_of_arbitrary_and_cut_input(hip, forward_outputs):
    """Random and flag-rich bytes at three capacities, and the forward outputs cut inside a literal run, behind 0xFC, inside a 0xFE run
    and in front of the length byte, or given a destination one byte short: the reference's ok flag, and its bytes when it accepts."""
    n_ok = 0
    recs = GOLDEN["inverse"] + GOLDEN["cut"]
    for rec in recs:
        if "cut" in rec:
            d = forward_outputs[json.dumps(rec["recipe"])][1][1][:rec["cut"]]
            assert md5(d) == rec["input_md5"]
        else:
            d = _input(rec)
        if len(d) == 0:
            continue
        ok, inv = hip.transform_inverse("LZP", d, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec["recipe"], rec["cap"], rec.get("where"))
        if rec["ok"]:
            n_ok += 1
            assert md5(inv) == rec["inv_md5"], ("inverse", rec["recipe"], rec["cap"])
            if "inv_hex" in rec:
                assert inv.hex() == rec["inv_hex"]
    assert 3 * n_ok >= len(recs)


@pytest.mark.parametrize("idx", range(len(lzp_cases.STREAM_CHAINS)))
def test_chain_bit_exact_and_decodes(hip, idx):
    """Eight blocks of 64 KiB (text with repeated paragraphs, random bytes that LZP skips, a constant block, period 5, one block twice,
    escapes, a tail of 10 bytes): the stream equals the reference's and decodes back in one call (decode ranges on)."""
    rec = GOLDEN["streams"][idx]
    data = lzp_cases.make(lzp_cases.STREAM)
    assert md5(data) == rec["input_md5"]
    bs = rec["block_size"]
    p = hip.params(rec["chain"], rec["entropy"], bs, checksum=rec["checksum"])
    cap = hip.encode_bound(p, len(data))
    d_in, d_out = hip.malloc(len(data) + 64), hip.malloc(cap)
    try:
        hip.h2d(d_in, data)
        bits = hip.encode_blocks(p, d_in, len(data), d_out, cap)
        enc = hip.d2h(d_out, (bits + 7) // 8)
        assert len(enc) == rec["stream_len"] and md5(enc) == rec["stream_md5"], rec["chain"]
        d_dec = hip.malloc(len(data) + bs + 64)
        try:
            ob, _, nb = hip.decode_blocks(p, d_out, bits, 0, d_dec, len(data) + bs)
            assert nb == 8 and hip.d2h(d_dec, ob) == data
        finally:
            hip.free(d_dec)
    finally:
        hip.free(d_in)
        hip.free(d_out)


@pytest.mark.parametrize("idx", range(len(GOLDEN["hosted"])))
def test_hosted_chain_bit_exact_and_decodes(tmp_path, idx):
    """TEXT on the host in front of LZP, BWT, RANK and ZRLT on the device, at 1 and 3 jobs: the .knz equals the reference's and decodes back."""
    import knzlib
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    rec = GOLDEN["hosted"][idx]
    data = lzp_cases.make(rec["recipe"])
    assert md5(data) == rec["input_md5"]
    bs = rec["block_size"]
    path = str(tmp_path / "s.knz")
    c = kz.Compressor(path, rec["chain"], rec["entropy"], bs, rec["jobs"], checksum=rec["checksum"])
    for off in range(0, len(data), bs):
        c.compress(data[off:off + bs])
    c.close()
    enc = open(path, "rb").read()
    assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"], (rec["chain"], rec["jobs"])
    d = kz.Decompressor(path, buffer_size=bs, jobs=rec["jobs"])
    out = bytearray()
    while True:
        chunk = d.decompress(bs)
        out += chunk
        if len(chunk) < bs:
            break
    d.close()
    assert bytes(out) == data


def test_cli_reads_and_writes_what_the_reference_does(tmp_path):
    """kanzi_amd_cli -c -t LZP+BWT+RANK+ZRLT -e ANS0 on about 300 KB: the reference's tool decodes it, and the other way round."""
    import knzlib
    ref_cli = os.path.join(knzlib.ROOT, "oracle", "_ref", "kanzi")
    if not os.path.exists(ref_cli):
        pytest.skip("the reference's command-line tool is not built (oracle/_ref/kanzi)")
    cli = os.path.join(knzlib.PKG, "kanzi_amd_cli")
    assert os.path.exists(cli), "run __graft_entry__.build()"
    data = _input(GOLDEN["cli"])
    src, ours, theirs, back = (str(tmp_path / n) for n in ("in.bin", "ours.knz", "theirs.knz", "back.bin"))
    open(src, "wb").write(data)
    args = ["-t", "LZP+BWT+RANK+ZRLT", "-e", "ANS0", "-b", "65536", "-j", "1"]
    p = subprocess.run([cli, "-c", "-i", src, "-o", ours, "-f"] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([ref_cli, "-c", "-i", src, "-o", theirs, "-f"] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert open(ours, "rb").read() == open(theirs, "rb").read()
    p = subprocess.run([ref_cli, "-d", "-i", ours, "-o", back, "-f", "-j", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and open(back, "rb").read() == data, p.stderr
    os.remove(back)
    p = subprocess.run([cli, "-d", "-i", theirs, "-o", back, "-f"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and open(back, "rb").read() == data, p.stderr
