"""UTF (UTFCodec, transform id 17) on the device: per stage through the C ABI, in whole chains through knz_hip_encode_blocks /
knz_hip_decode_blocks, in a .knz file with and without TEXT on the host in front, and through the command-line tool. Expected results
come from tests/golden/utf.json (written from the reference by tools/make_utf_golden.py)."""
import hashlib
import importlib
import json
import os
import subprocess

import pytest

import utf_cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "utf.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def _input(rec):
    d = utf_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["recipe"]
    return d


@pytest.fixture(scope="module")
def forward_outputs(hip):
    """The device's forward result (ok, bytes, data type afterwards) of every stage record, by index, computed once."""
    out = []
    for rec in GOLDEN["stage"]:
        d = _input(rec)
        out.append((d, hip.transform_forward_dt("UTF", d, rec["cap"], rec["dtype"])))
    return out


def test_stage_forward_golden_and_round_trip(hip, forward_outputs):
    """Lengths around the guard and the tail, every start offset and overrun, the BOM, preset data types, text that validation or the size
    estimate refuses, 200 to 40,000 distinct symbols (two-byte aliases whose second byte is >= 0x80; 32,768 and more refused with the type
    left at UTF8), bytes that only an unvalidated block may hold (0xC0 as a lead, broken second and third bytes), the symbol walk ending
    at a chunk border -1, +0, +1, +3 and a block of more than 256 chunks."""
    for rec, (d, (ok, fwd, dt)) in zip(GOLDEN["stage"], forward_outputs):
        if len(d) == 0:
            assert ok and fwd == b""
            continue
        assert int(ok) == rec["ok"], ("ok", rec["recipe"], rec["dtype"])
        assert dt == rec["dtype_out"], ("data type", rec["recipe"], rec["dtype"])
        if not rec["ok"]:
            continue
        assert len(fwd) == rec["fwd_len"] and md5(fwd) == rec["fwd_md5"], ("forward", rec["recipe"])
        if rec["recipe"] == utf_cases.LOSSY:
            continue                                         # (the reference does not give this block back either)
        ok, back = hip.transform_inverse("UTF", fwd, len(d) + 1)
        assert ok and back == d, ("round trip", rec["recipe"])


def test_stage_without_a_data_type_starts_undefined(hip):
    """knz_hip_transform_forward has no Context: validation runs, as for UNDEFINED."""
    d = utf_cases.make(utf_cases.CAP_CASE)
    ok, fwd = hip.transform_forward("UTF", d, len(d) + 8192)
    assert ok and (ok, fwd, 8) == hip.transform_forward_dt("UTF", d, len(d) + 8192, 0)
    ok, _ = hip.transform_forward("UTF", utf_cases.make(["plant", 7200, 0, utf_cases._BASE, 300, "c04142"]), 7200 + 8192)
    assert not ok


def test_stage_refuses_short_destination(hip):
    """UTFCodec.cpp:62: a destination one byte below getMaxEncodedLength (count + 8192) is refused and the type stays, the bound is enough."""
    d = utf_cases.make(utf_cases.CAP_CASE)
    ok, _, dt = hip.transform_forward_dt("UTF", d, len(d) + 8191, 0)
    assert not ok and dt == 0
    ok, _, dt = hip.transform_forward_dt("UTF", d, len(d) + 8192, 0)
    assert ok and dt == 8


def test_stage_inverse_of_whole_damaged_and_arbitrary_input(hip, forward_outputs):
    """Every accepted output into len (refused), len + 1 and len + 1000 bytes; outputs cut by a byte, in the map and mid-stream, with
    n = 0, another header byte 1, an alias >= n, a map entry of no size class; random bytes: the reference's ok flag, and its bytes when
    it accepts."""
    n_ok = 0
    recs = GOLDEN["inverse"] + GOLDEN["damaged"]
    for rec in recs:
        if "stage" in rec:
            d = forward_outputs[rec["stage"]][1][1]
            if "op" in rec:
                d = utf_cases.damage(d, rec["op"])
        else:
            d = _input(rec)
        assert md5(d) == rec["input_md5"]
        ok, inv = hip.transform_inverse("UTF", d, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec.get("stage"), rec.get("op"), rec.get("recipe"), rec["cap"])
        if rec["ok"]:
            n_ok += 1
            assert len(inv) == rec["inv_len"] and md5(inv) == rec["inv_md5"], ("inverse", rec.get("stage"), rec.get("op"), rec["cap"])
            if "inv_hex" in rec:
                assert inv.hex() == rec["inv_hex"]
    assert 3 * n_ok >= len(recs)


@pytest.mark.parametrize("idx", range(len(utf_cases.STREAM_CHAINS)))
def test_chain_bit_exact_and_decodes(hip, idx):
    """Eight blocks of 64 KiB cut through code points (utf8, ASCII text that UTF refuses, random bytes, a repeated block, 5,000 distinct
    symbols) and a tail of 10 bytes: the stream equals the reference's headerless stream and decodes back in one call."""
    rec = GOLDEN["streams"][idx]
    data = utf_cases.make(utf_cases.STREAM)
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
            assert nb == 9 and hip.d2h(d_dec, ob) == data
        finally:
            hip.free(d_dec)
    finally:
        hip.free(d_in)
        hip.free(d_out)


@pytest.mark.parametrize("idx", range(len(GOLDEN["hosted"])))
def test_knz_file_bit_exact_and_decodes(tmp_path, idx):
    """TEXT on the host with UTF, BWT, RANK and ZRLT on the device behind it, and UTF + BWT + SRT + ZRLT with no host stage, at 1 and 3
    jobs, on blocks TEXT takes, blocks UTF takes and blocks neither takes: the .knz equals the reference's and decodes back."""
    import knzlib
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    rec = GOLDEN["hosted"][idx]
    data = utf_cases.make(utf_cases.HOSTED_INPUT)
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
    """kanzi_amd_cli -c -t LZP+UTF+BWT+RANK+ZRLT -e ANS0 on about 300 KB: the reference's tool decodes it, and the other way round."""
    import knzlib
    ref_cli = os.path.join(knzlib.ROOT, "oracle", "_ref", "kanzi")
    if not os.path.exists(ref_cli):
        pytest.skip("the reference's command-line tool is not built (oracle/_ref/kanzi)")
    cli = os.path.join(knzlib.PKG, "kanzi_amd_cli")
    assert os.path.exists(cli), "run __graft_entry__.build()"
    data = _input(GOLDEN["cli"])
    src, ours, theirs, back = (str(tmp_path / n) for n in ("in.bin", "ours.knz", "theirs.knz", "back.bin"))
    open(src, "wb").write(data)
    args = utf_cases.CLI_ARGS + ["-b", "65536", "-j", "1"]
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
