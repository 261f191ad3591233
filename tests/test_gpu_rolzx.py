"""ROLZX (ROLZCodec2, transform id 12) on the device: per stage through the C ABI, in whole chains through knz_hip_encode_blocks /
knz_hip_decode_blocks, in a .knz file with a host stage in front, through the C++ mirror and through the command-line tool. Expected
results come from tests/golden/rolzx.json (tools/make_rolzx_golden.py): stage and damaged records from the model that
tests/test_rolzx_model.py pins to the reference, stream, hosted and chunk records from the reference itself."""
import hashlib
import importlib
import json
import os
import subprocess

import pytest

import rolzx_cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rolzx.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def _input(rec):
    d = rolzx_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["recipe"]
    return d


@pytest.fixture(scope="module")
def forward_outputs(hip):
    """The device's forward result of every stage record, computed once: (input, ok, bytes, data type left)."""
    out = []
    for rec in GOLDEN["stage"]:
        d = _input(rec)
        out.append((d,) + tuple(hip.transform_forward_dt("ROLZX", d, rec["cap"], rec["dtype_in"])))
    return out


def test_stage_forward_golden_and_round_trip(hip, forward_outputs):
    """Lengths 0, 63 (refused), 64, 65 and 72; matches of minMatch - 1 (none), minMatch and the maximum; a longer candidate behind one
    that reaches maxMatch exactly; two candidates of equal length; keys with more than 32 positions; a position whose hash32 is 0 in a
    ring of zero entries (a match with position 0); match attempts in the last 8 bytes; random bytes (refused: no gain); DNA (getKey2,
    matches of 7 and more) and EXE (keys 3 bytes back) detected and preset, with the type read back."""
    for rec, (d, ok, fwd, dt) in zip(GOLDEN["stage"], forward_outputs):
        if len(d) == 0:
            assert ok and fwd == b""
            continue
        assert int(ok) == rec["ok"], ("ok", rec["recipe"][:3], rec["dtype_in"])
        assert dt == rec["dtype_out"], ("data type", rec["recipe"][:3], rec["dtype_in"])
        if not rec["ok"]:
            continue
        assert len(fwd) == rec["fwd_len"] and md5(fwd) == rec["fwd_md5"], ("forward", rec["recipe"][:3], rec["dtype_in"])
        ok, back = hip.transform_inverse("ROLZX", fwd, len(d))
        assert ok and back == d, ("round trip", rec["recipe"][:3], rec["dtype_in"])


def test_stage_without_a_context_starts_undefined(hip, forward_outputs):
    """knz_hip_transform_forward has no Context: a fresh UNDEFINED one per block, so DNA is still detected."""
    for rec, (d, ok, fwd, _) in zip(GOLDEN["stage"], forward_outputs):
        if rec["recipe"][:3] in (["dna", 3000, 51], ["text", 4097, 11]) and rec["dtype_in"] == 0:
            ok2, fwd2 = hip.transform_forward("ROLZX", d, rec["cap"])
            assert ok2 and fwd2 == fwd


def test_stage_refuses_short_destination(hip):
    """ROLZCodec.cpp:916: a destination one byte below getMaxEncodedLength is refused, the bound itself is enough."""
    d = rolzx_cases.make(rolzx_cases.SHORT_CAP)
    ok, _ = hip.transform_forward("ROLZX", d, rolzx_cases.max_encoded(len(d)) - 1)
    assert not ok
    ok, _ = hip.transform_forward("ROLZX", d, rolzx_cases.max_encoded(len(d)))
    assert ok


def test_stage_inverse_of_cut_and_damaged_input(hip, forward_outputs):
    """Forward outputs whole, cut inside the first 8 literals, mid-stream and 1 to 4 bytes before the end, with a byte flipped, and
    with a length field above the capacity: the model's verdict, and its bytes where it accepts."""
    outputs = {json.dumps(rec["recipe"]): fwd for rec, (_, ok, fwd, _) in zip(GOLDEN["stage"], forward_outputs) if ok and rec["dtype_in"] == 0}
    n_refused = 0
    for rec in GOLDEN["damaged"]:
        bad = rolzx_cases.damage(outputs[json.dumps(rec["recipe"])], rec["op"])
        assert md5(bad) == rec["input_md5"], (rec["recipe"][:3], rec["op"])
        ok, inv = hip.transform_inverse("ROLZX", bad, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec["recipe"][:3], rec["op"], rec["cap"])
        n_refused += 0 if ok else 1
        if rec["ok"]:
            assert md5(inv) == rec["inv_md5"], ("inverse", rec["recipe"][:3], rec["op"], rec["cap"])
    assert n_refused > 0


def _stream(hip, chain, entropy, bs, checksum, data, rec, n_blocks):
    p = hip.params(chain, entropy, bs, checksum=checksum)
    cap = hip.encode_bound(p, len(data))
    d_in, d_out = hip.malloc(len(data) + 64), hip.malloc(cap)
    try:
        hip.h2d(d_in, data)
        bits = hip.encode_blocks(p, d_in, len(data), d_out, cap)
        enc = hip.d2h(d_out, (bits + 7) // 8)
        assert len(enc) == rec["stream_len"] and md5(enc) == rec["stream_md5"], chain
        d_dec = hip.malloc(len(data) + bs + 64)
        try:
            ob, _, nb = hip.decode_blocks(p, d_out, bits, 0, d_dec, len(data) + bs)
            return nb == n_blocks and hip.d2h(d_dec, ob) == data
        finally:
            hip.free(d_dec)
    finally:
        hip.free(d_in)
        hip.free(d_out)


def test_ragged_batch_bit_exact_and_decodes(hip):
    """71 blocks of 4,096 bytes (the last one 100) in one batch, no two neighbours alike: every kind of stage record filled up with
    text, DNA, ELF, random, periodic and constant blocks. The stream equals the reference's and decodes back."""
    rec = GOLDEN["ragged"]
    data = rolzx_cases.make(rolzx_cases.RAGGED)
    assert md5(data) == rec["input_md5"]
    assert _stream(hip, "ROLZX", "NONE", rec["block_size"], 0, data, rec, 71)


def test_ragged_batch_in_slices(hip, monkeypatch):
    """The same batch with the tables limited to 7 blocks at a time (KNZ_ROLZX_TABLES_MAX): eleven slices, the same stream."""
    monkeypatch.setenv("KNZ_ROLZX_TABLES_MAX", str(7 * 8667136))
    rec = GOLDEN["ragged"]
    data = rolzx_cases.make(rolzx_cases.RAGGED)
    assert _stream(hip, "ROLZX", "NONE", rec["block_size"], 0, data, rec, 71)


@pytest.mark.parametrize("idx", range(len(rolzx_cases.CHUNKS)))
def test_chunks_of_16_mib(hip, idx):
    """Blocks of 16 MiB, 16 MiB + 1, + 12 and + 100,000 bytes of a short repeated text (32 MiB block size): the stream equals the
    reference's; decoding gives the input back where the reference decodes its own output, and fails or gives other bytes where it does
    not (16 MiB + 1: the decoder cuts chunks by the full length, the encoder by the length less 4)."""
    rec = GOLDEN["chunks"][idx]
    data = _input(rec)
    try:
        same = _stream(hip, "ROLZX", "NONE", rec["block_size"], 0, data, rec, 1)
    except AssertionError:
        raise
    except Exception:                                        # (the library reports the refused inverse)
        same = False
    assert same == bool(rec["reference_decodes_it"])


@pytest.mark.parametrize("idx", range(len(rolzx_cases.STREAM_CHAINS)))
def test_chain_bit_exact_and_decodes(hip, idx):
    """Eight blocks of 64 KiB (text, random bytes that ROLZX refuses, DNA, an ELF block, text again, a long period, four symbols, a tail
    of 10 bytes) through ROLZX / NONE, ROLZX / HUFFMAN, PACK+ROLZX / ANS0, ROLZX+RLT / FPAQ (the type ROLZX writes reaches RLT) and
    ROLZX / ANS0 with checksums: the stream equals the reference's and decodes back in one call."""
    rec = GOLDEN["streams"][idx]
    data = rolzx_cases.make(rolzx_cases.STREAM)
    assert md5(data) == rec["input_md5"]
    assert _stream(hip, rec["chain"], rec["entropy"], rec["block_size"], rec["checksum"], data, rec, 8)


@pytest.mark.parametrize("idx", range(len(GOLDEN["hosted"])))
def test_hosted_chain_bit_exact_and_decodes(tmp_path, idx):
    """TEXT on the host in front of ROLZX on the device, at 1 and 3 jobs: the .knz equals the reference's and decodes back."""
    import knzlib
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    rec = GOLDEN["hosted"][idx]
    data = _input(rec)
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


def test_cpp_rolzx_mirror():
    """ROLZCodec of include/kanzi_amd.hpp: the constructors and the refusal of ROLZ, getMaxEncodedLength, the data type written back, round
    trips directly, through TransformFactory and through the stream classes (tests/cpp/rolzx_mirror_test.cpp)."""
    import knzlib
    exe = os.path.join(knzlib.ROOT, "tests", "cpp", "rolzx_mirror_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_cli_reads_and_writes_what_the_reference_does(tmp_path):
    """kanzi_amd_cli -c -t ROLZX -e HUFFMAN on about 300 KB: byte-identical to the reference tool's file, each tool reads the other's;
    -t ROLZ is still refused, with a message that names it."""
    import knzlib
    ref_cli = os.path.join(knzlib.ROOT, "oracle", "_ref", "kanzi")
    if not os.path.exists(ref_cli):
        pytest.skip("the reference's command-line tool is not built (oracle/_ref/kanzi)")
    cli = os.path.join(knzlib.PKG, "kanzi_amd_cli")
    assert os.path.exists(cli), "run __graft_entry__.build()"
    data = _input(GOLDEN["cli"])
    src, ours, theirs, back = (str(tmp_path / n) for n in ("in.bin", "ours.knz", "theirs.knz", "back.bin"))
    open(src, "wb").write(data)
    args = ["-t", "ROLZX", "-e", "HUFFMAN", "-b", "65536", "-j", "1"]
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
    for chain in ("ROLZ", "TEXT+ROLZ"):
        p = subprocess.run([cli, "-c", "-i", src, "-o", ours, "-f", "-t", chain, "-e", "NONE"], capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "ROLZ transform" in p.stderr, p.stderr
