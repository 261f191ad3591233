"""TPAQ and TPAQX (entropy ids 7 and 9) on the device: whole streams against the reference's digests in tests/golden/tpaq.json
(tools/make_tpaq_golden.py), per stage through the C ABI against tests/tpaq_model.py (pinned to the reference by
tests/test_tpaq_model.py), a states table small enough for pointers of different contexts to meet, a batch that runs in slices of
tables, the second staging tier, refusals, and the host interfaces."""
import hashlib
import importlib
import json
import os
import subprocess

import pytest

import knzlib
import tpaq_cases
import tpaq_model

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tpaq.json")))
MIB = 1 << 20


def md5(b):
    return hashlib.md5(b).hexdigest()


def _input(rec):
    d = tpaq_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["name"]
    return d


def _header(rec):
    knzlib.load_pkg()
    framing = importlib.import_module("kanzi_amd.framing")
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    hdr, bits = framing.make_header(tpaq_cases.ENTROPY_ID[rec["coder"]], hipapi.transform_type(rec["chain"]), rec["block_size"], rec["checksum"], rec["orig_size"])
    assert bits == rec["header_bits"] and hdr.hex() == rec["header_hex"]
    return hdr, bits


def _shift5(enc):
    return (((0x1F << (8 * len(enc))) | int.from_bytes(enc, "big")) << 3).to_bytes(len(enc) + 1, "big")


def _rec(kind, name, coder):
    return next(r for r in GOLDEN[kind] if r["name"] == name and r["coder"] == coder)


def _stream_check(hip, rec, cap=None):
    """The record's stream through knz_hip_encode_blocks, compared and decoded back from the bit behind the header."""
    data = _input(rec)
    bs = rec["block_size"]
    hdr, hbits = _header(rec)
    p = hip.params(rec["chain"], rec["coder"], bs, checksum=rec["checksum"])
    cap = cap or hip.encode_bound(p, len(data))
    d_in, d_out, d_dec = hip.malloc(len(data) + 64), hip.malloc(cap), hip.malloc(len(data) + bs + 64)
    try:
        hip.h2d(d_in, data)
        bits = hip.encode_blocks(p, d_in, len(data), d_out, cap, prologue=hdr, prologue_bits=hbits)
        enc = hip.d2h(d_out, (bits + 7) // 8)
        assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]
        ob, _, nb = hip.decode_blocks(p, d_out, bits, hbits, d_dec, len(data) + bs)
        assert nb == (len(data) + bs - 1) // bs and hip.d2h(d_dec, ob) == data
    finally:
        for ptr in (d_in, d_out, d_dec):
            hip.free(ptr)


RECORDS = [(k, i) for k in ("streams", "chains") for i in range(len(GOLDEN[k]))]


@pytest.mark.parametrize("kind,idx", RECORDS, ids=["%s-%s" % (GOLDEN[k][i]["name"], GOLDEN[k][i]["coder"]) for k, i in RECORDS])
def test_stream_is_the_references_and_decodes(hip, kind, idx):
    """knz_hip_encode_blocks behind the stream header writes the reference's bytes, bit for bit, for every record and both coders:
    copy blocks and the first coded length, a match that reaches 88 and is cleared, mostly binary input and input that crosses both
    _binCount thresholds, every tier of the states table (block sizes 1024 to 64 MiB), masks that are not 2^k - 1 (-b 10000), ragged
    batches with both checksums, and RLT, BWT+RANK+ZRLT and LZP in front. knz_hip_decode_blocks gives the input back from the non-zero
    start bit behind the header; the eight blocks of the BWT record are decoded in three lanes, each with tables of its own."""
    _stream_check(hip, GOLDEN[kind][idx])


STAGE = [(n, r, bs) for n, r, bs, ck in tpaq_cases.STREAMS if n in ("len16", "len17", "len65", "len4097", "const", "random", "pairs", "bs10000", "bs4m")]


@pytest.mark.parametrize("coder", tpaq_cases.CODERS)
@pytest.mark.parametrize("name,recipe,bs", STAGE, ids=[s[0] for s in STAGE])
def test_stage_entry_point_matches_model_and_decodes(hip, name, recipe, bs, coder):
    """knz_hip_entropy_encode_bs / _decode_bs, the per-stage calls that carry the stream's block size: the bits are the model's for the
    same block size, and they decode back with every bit used, from bit 0 and from bit 5. (bs10000 is longer than its block size: a
    buffer that wraps through masks 9,999 and 16 n - 1.)"""
    data = tpaq_cases.make(recipe)
    x = tpaq_cases.EXTRA[coder]
    enc, bits = tpaq_model.encode(data, x, bs)
    got, gbits = hip.entropy_encode(coder, data, stream_block_size=bs)
    assert gbits == bits and got == enc
    n, back, used = hip.entropy_decode(coder, got, len(data), in_bits=gbits, stream_block_size=bs)
    assert n == len(data) and back == data and used == bits
    n, back, used = hip.entropy_decode(coder, _shift5(enc), len(data), start_bit=5, in_bits=5 + bits, stream_block_size=bs)
    assert n == len(data) and back == data and used == bits


def test_stage_entry_point_without_a_block_size(hip):
    """knz_hip_entropy_encode / _decode_v have no block size to pass: they take the buffer's length rounded up to 16, as the header says."""
    data = tpaq_cases.make(["text", 3000, 2])
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    import ctypes as C
    for coder in tpaq_cases.CODERS:
        e = hipapi.ENTROPY_IDS[coder]
        out = (C.c_uint8 * (40 * len(data)))()
        bits = C.c_uint64(0)
        assert hip.L.knz_hip_entropy_encode(hip.h, e, data, len(data), out, len(out), C.byref(bits)) == 0
        want = tpaq_model.encode(data, tpaq_cases.EXTRA[coder], (len(data) + 15) & ~15)
        assert (C.string_at(out, (bits.value + 7) // 8), bits.value) == want
        n, back, used = hip.entropy_decode(coder, want[0], len(data), in_bits=want[1])
        assert n == len(data) and back == data and used == want[1]


@pytest.mark.parametrize("coder", tpaq_cases.CODERS)
def test_small_states_table_where_pointers_meet(hip, monkeypatch, coder):
    """KNZ_TPAQ_STATES_LOG=12: the big states table has 4,096 bytes, so the pointers of contexts 2 to 6 meet in one cell all the time
    (a cell shared by m pointers is stepped m times; TPAQX steps the seventh behind the reads of the others). The bits are those of
    the model with the same table size."""
    monkeypatch.setenv("KNZ_TPAQ_STATES_LOG", "12")
    x = tpaq_cases.EXTRA[coder]
    for recipe in (["text", 6000, 4], ["hibit", 3000, 5, 40]):
        data = tpaq_cases.make(recipe)
        want = tpaq_model.encode(data, x, MIB, states_log=12)
        got = hip.entropy_encode(coder, data, stream_block_size=MIB)
        assert got == want
        n, back, used = hip.entropy_decode(coder, got[0], len(data), in_bits=got[1], stream_block_size=MIB)
        assert n == len(data) and back == data and used == got[1]


def test_batch_runs_in_slices_of_tables(hip, monkeypatch):
    """KNZ_TPAQ_TABLES_MAX below the tables of the batch: the six blocks of the bs1024 record run two at a time (TPAQ: about 20 MiB of
    tables per block, 50 MB allowed) and one at a time (TPAQX: about 32 MiB, 40 MB allowed), encoder and decoder, every block with
    tables of the format's size: the stream is still the reference's."""
    for coder, budget, launches in (("TPAQ", 50_000_000, 3), ("TPAQX", 40_000_000, 6)):
        monkeypatch.setenv("KNZ_TPAQ_TABLES_MAX", str(budget))
        rec = _rec("streams", "bs1024", coder)
        hip.set_profiling(True)
        try:
            _stream_check(hip, rec)
            times = {k[0]: k[2] for k in hip.kernel_times()}       # (of the last call, the decode)
        finally:
            hip.set_profiling(False)
        assert times.get("k_tpaq_decode") == launches, times


def test_second_tier_with_the_first_lowered(hip, monkeypatch):
    """KNZ_CM_TIER1_DIV=4 makes the first tier n / 4 (first staging and knz_hip_encode_bound alike), as for CM: the record of 8,000 random bytes is
    coded a second time into 32 n + 16 bytes; an output buffer of the first tier is refused with code 12 and one of the second tier
    takes the reference's stream; the per-stage entry point, the sharded run encoder and the C++ mirror retry by themselves."""
    monkeypatch.setenv("KNZ_CM_TIER1_DIV", "4")
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    sharded = importlib.import_module("kanzi_amd.sharded")
    for coder in tpaq_cases.CODERS:
        rec = _rec("streams", "random8k", coder)
        d = _input(rec)
        p = hip.params("NONE", coder, rec["block_size"])
        cap = hip.encode_bound(p, len(d))
        assert cap < rec["knz_len"]
        hdr, hbits = _header(rec)
        d_in, d_out = hip.malloc(len(d) + 64), hip.malloc(cap)
        try:
            hip.h2d(d_in, d)
            with pytest.raises(hipapi.KnzError) as e:
                hip.encode_blocks(p, d_in, len(d), d_out, cap, prologue=hdr, prologue_bits=hbits)
            assert e.value.code == 12
        finally:
            hip.free(d_in)
            hip.free(d_out)
        _stream_check(hip, rec, cap + 32 * len(d))
        _stream_check(hip, _rec("streams", "blocks_x32", coder), None)        # two blocks in one batch, inside the lowered bound
        hip.set_profiling(True)
        try:
            got = hip.entropy_encode(coder, d, stream_block_size=MIB)
            launches = sum(k[2] for k in hip.kernel_times() if k[0] == "k_tpaq_encode")
        finally:
            hip.set_profiling(False)
        assert got == tpaq_model.encode(d, tpaq_cases.EXTRA[coder], MIB) and launches >= 2
        enc, bits = sharded.DeviceRunEncoder(0, "NONE", coder, rec["block_size"], orig_size=rec["orig_size"])(d, 0, True, True)
        assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]
    exe = os.environ.get("KNZ_TEST_TPAQ_MIRROR_EXE") or os.path.join(knzlib.ROOT, "tests", "cpp", "tpaq_mirror_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, KNZ_CM_TIER1_DIV="4"))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_refusals_leave_the_context_healthy(hip):
    """A payload cut at several bit positions and a var-int above 32 bytes per byte are refused (-1 from the per-stage call); a block
    longer than the tables were laid out for cannot be asked for; bitstream version 7 is refused; a good block decodes after each."""
    data = tpaq_cases.make(["text", 2000, 4])
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    for coder in tpaq_cases.CODERS:
        x = tpaq_cases.EXTRA[coder]
        enc, bits = tpaq_model.encode(data, x, MIB)
        for cut in (0, 1, 8, 55, 56, bits // 2, bits - 57, bits - 1):
            n, _, used = hip.entropy_decode(coder, enc[:(cut + 7) // 8] or b"\0", len(data), in_bits=cut, stream_block_size=MIB)
            assert n == -1 and used <= cut
            n, back, _ = hip.entropy_decode(coder, enc, len(data), in_bits=bits, stream_block_size=MIB)
            assert n == len(data) and back == data
        bw = tpaq_model.BitWriter()
        tpaq_model.put_varint(bw, (100 << 5) + 1)
        bw.put(0, 56 + 8 * 40)
        n, _, _ = hip.entropy_decode(coder, bw.bytes(), 100, in_bits=bw.n, stream_block_size=MIB)
        assert n == -1
        with pytest.raises(hipapi.KnzError):
            hip.entropy_decode(coder, enc, len(data), in_bits=bits, bs_version=7, stream_block_size=MIB)
        n, back, _ = hip.entropy_decode(coder, enc, len(data), in_bits=bits, stream_block_size=MIB)
        assert n == len(data) and back == data


def _host_cases():
    return [r for r in GOLDEN["streams"] if r["name"] in ("blocks_x32", "bs10000", "len2")] + GOLDEN["chains"] + GOLDEN["hosted"]


@pytest.mark.parametrize("rec", _host_cases(), ids=lambda r: "%s-%s" % (r["name"], r["coder"]))
def test_python_compressor_writes_and_reads_the_reference_file(tmp_path, rec):
    """kz.Compressor(..., entropy="TPAQ" / "TPAQX") through the C API: the reference's .knz byte for byte (TEXT, in variant 1, on the
    host in the last two cases, UTF behind it on the device), and kz.Decompressor reads it back. The C API's compressor is handed no
    input size, so the golden stream is the one the reference writes when it reads standard input."""
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    data = _input(rec)
    bs = rec["block_size"]
    path = str(tmp_path / "s.knz")
    c = kz.Compressor(path, rec["chain"], rec["coder"], bs, 1, checksum=rec["checksum"])
    for off in range(0, len(data), bs):
        c.compress(data[off:off + bs])
    c.close()
    enc = open(path, "rb").read()
    assert len(enc) == rec["unsized_len"] and md5(enc) == rec["unsized_md5"]
    d = kz.Decompressor(path, buffer_size=bs, jobs=1)
    out = bytearray()
    while True:
        chunk = d.decompress(bs)
        out += chunk
        if len(chunk) < bs:
            break
    d.close()
    assert bytes(out) == data


def test_cli_writes_and_reads_the_reference_file(tmp_path):
    """kanzi_amd_cli -c -e TPAQ / TPAQX: the reference's files (-t RLT among them), and -d reads them back."""
    cli = os.environ.get("KNZ_TEST_CLI", os.path.join(knzlib.PKG, "kanzi_amd_cli"))
    for rec in [r for r in _host_cases() if r["name"] in ("blocks_x32", "RLT", "TEXT+UTF+BWT+RANK+ZRLT")]:
        data = _input(rec)
        src, out, back = str(tmp_path / "in.bin"), str(tmp_path / "out.knz"), str(tmp_path / "back.bin")
        open(src, "wb").write(data)
        extra = ["-x%d" % rec["checksum"]] if rec["checksum"] else []
        p = subprocess.run([cli, "-c", "-i", src, "-o", out, "-f", "-t", rec["chain"], "-e", rec["coder"], "-b", str(rec["block_size"]), "-j", "1"] + extra,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        enc = open(out, "rb").read()
        assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"], rec["name"]
        p = subprocess.run([cli, "-d", "-i", out, "-o", back, "-f"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        assert open(back, "rb").read() == data


def test_cpp_tpaq_mirror():
    """TPAQPredictor / BinaryEntropyEncoder / BinaryEntropyDecoder of include/kanzi_amd.hpp: round trips directly, through the factories
    and the stream classes, the block size reaching the device, and the refused constructor arguments (tests/cpp/tpaq_mirror_test.cpp)."""
    exe = os.environ.get("KNZ_TEST_TPAQ_MIRROR_EXE") or os.path.join(knzlib.ROOT, "tests", "cpp", "tpaq_mirror_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
