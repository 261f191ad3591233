"""CM (entropy id 6) on the device: per stage through the C ABI against tests/cm_model.py (pinned to the reference by
tests/test_cm_model.py), whole streams against the reference's digests in tests/golden/cm.json (tools/make_cm_golden.py), a batch with
more blocks than compute units, refusals of damaged streams, and the host interfaces."""
import hashlib
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import cm_cases
import cm_model
import knzlib

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cm.json")))
ERR_PROCESS_BLOCK = 13


def md5(b):
    return hashlib.md5(b).hexdigest()


def _input(rec):
    d = cm_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["name"]
    return d


def _header(rec, chain="NONE"):
    knzlib.load_pkg()
    framing = importlib.import_module("kanzi_amd.framing")
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    hdr, bits = framing.make_header(6, hipapi.transform_type(chain), rec["block_size"], rec["checksum"], rec["orig_size"])
    assert bits == rec["header_bits"]
    return hdr, bits


def _shift5(enc):
    return (((0x1F << (8 * len(enc))) | int.from_bytes(enc, "big")) << 3).to_bytes(len(enc) + 1, "big")


STAGE = [(n, r) for n, r, bs, ck in cm_cases.STREAMS if bs == 1 << 20]


@pytest.mark.parametrize("name,recipe", STAGE, ids=[n for n, _ in STAGE])
def test_stage_encode_matches_model_and_decodes(hip, name, recipe):
    """knz_hip_entropy_encode / _decode: lengths 1 to 4,097, var-ints of 1, 2 and 3 bytes, constant blocks, runMask off and on, every
    row, random bytes, text, the adversary (which stays inside the first staging, as the fixture records): the bits are the model's,
    and they decode back with every bit used, from bit 0 and from bit 5."""
    data = cm_cases.make(recipe)
    enc, bits = cm_model.encode(data)
    got, gbits = hip.entropy_encode("CM", data)
    assert gbits == bits and got == enc
    n, back, used = hip.entropy_decode("CM", got, len(data), in_bits=gbits)
    assert n == len(data) and back == data and used == bits
    n, back, used = hip.entropy_decode("CM", _shift5(enc), len(data), start_bit=5, in_bits=5 + bits)
    assert n == len(data) and back == data and used == bits


def test_adversary_takes_the_path_the_fixture_says(hip):
    """The fixture records that the adversary block's payload (8,424 bytes) stays below the first staging of n + n / 8 = 9,216 bytes:
    the block is coded once, inside knz_hip_encode_bound, and equals the reference's stream. (The second pass is covered by the
    emulator test, tests/test_emu_cm.py.)"""
    a = GOLDEN["adversary"]
    assert a["exceeds_first_staging"] is False and a["payload_bytes"] <= a["first_staging"]
    rec = next(r for r in GOLDEN["streams"] if r["name"] == "adversary")
    d = _input(rec)
    p = hip.params("NONE", "CM", rec["block_size"])
    assert hip.encode_bound(p, len(d)) >= a["payload_bytes"] + 64
    hip.set_profiling(True)
    try:
        got, gbits = hip.entropy_encode("CM", d)
        launches = sum(k[2] for k in hip.kernel_times() if k[0] == "k_cm_encode")
    finally:
        hip.set_profiling(False)
    assert launches == 1
    assert (got, gbits) == cm_model.encode(d)


@pytest.mark.parametrize("kind,idx", [(k, i) for k in ("streams", "chains") for i in range(len(GOLDEN[k]))],
                         ids=[r["name"] for k in ("streams", "chains") for r in GOLDEN[k]])
def test_stream_is_the_references_and_decodes(hip, kind, idx):
    """knz_hip_encode_blocks behind the stream header writes the reference's bytes (one block and several of different lengths,
    checksums 32 and 64, copy blocks, BWT+RANK+ZRLT, BWT+MTFT+ZRLT and LZP in front); knz_hip_decode_blocks gives the input back from
    the non-zero start bit behind the header."""
    rec = GOLDEN[kind][idx]
    data = _input(rec)
    bs = rec["block_size"]
    hdr, hbits = _header(rec, rec["chain"])
    p = hip.params(rec["chain"], "CM", bs, checksum=rec["checksum"])
    cap = hip.encode_bound(p, len(data))
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


def test_more_blocks_than_compute_units(hip):
    """300 blocks of 2 KiB, the last one short: a workgroup holds the predictor in 150 KB of LDS, so one runs per compute unit and the
    rest of the batch queues. The stream equals the model's block for block and decodes back."""
    bs = 2048
    data = cm_cases.make(["mixed", 299 * bs + 777, 5])
    knzlib.load_pkg()
    framing = importlib.import_module("kanzi_amd.framing")
    hdr, hbits = framing.make_header(6, 0, bs, 0, len(data))
    want = cm_model.stream(hdr, hbits, data, bs)
    p = hip.params("NONE", "CM", bs)
    cap = hip.encode_bound(p, len(data))
    d_in, d_out, d_dec = hip.malloc(len(data) + 64), hip.malloc(cap), hip.malloc(len(data) + bs + 64)
    try:
        hip.h2d(d_in, data)
        bits = hip.encode_blocks(p, d_in, len(data), d_out, cap, prologue=hdr, prologue_bits=hbits)
        enc = hip.d2h(d_out, (bits + 7) // 8)
        assert enc == want
        ob, _, nb = hip.decode_blocks(p, d_out, bits, hbits, d_dec, len(data) + bs)
        assert nb == 300 and hip.d2h(d_dec, ob) == data
    finally:
        for ptr in (d_in, d_out, d_dec):
            hip.free(ptr)


def _bad_then_good(hip, stream, bits, count, want=None):
    n, back, used = hip.entropy_decode("CM", stream, count, in_bits=bits)
    assert used <= bits
    if want is None:
        assert n == -1
    else:
        assert n == -1 or (n == count and (not isinstance(want, bytes) or back == want))
    good = cm_cases.make(["geom", 127, 105, 30])
    enc, gbits = cm_model.encode(good)
    n, back, _ = hip.entropy_decode("CM", enc, len(good), in_bits=gbits)
    assert n == len(good) and back == good


def test_refusals_leave_the_context_healthy(hip):
    """A payload cut at several bit positions and var-ints above 32 bytes per byte or past the end are refused (the per-stage call
    reports -1, the block call code 13); a flipped bit is refused or decodes to what the model decodes; a good block decodes right
    after every one of them."""
    data = cm_cases.make(["text", 3003, 4])
    enc, bits = cm_model.encode(data)
    for cut in (0, 1, 7, 8, 55, 56, bits // 2, bits - 57, bits - 1):
        _bad_then_good(hip, enc[:(cut + 7) // 8] or b"\0", cut, len(data))
    rng = np.random.default_rng(6)
    for _ in range(6):
        d = bytearray(enc)
        at = int(rng.integers(0, bits))
        d[at >> 3] ^= 0x80 >> (at & 7)
        try:
            want = cm_model.decode(bytes(d), len(data), 0, bits)[0]
        except ValueError:
            want = None
        _bad_then_good(hip, bytes(d), bits, len(data), want)
    for n, size in ((100, (100 << 5) + 1), (100, 3000)):
        bw = cm_model.BitWriter()
        cm_model.put_varint(bw, size)
        bw.put(0, 56 + 8 * 40)
        _bad_then_good(hip, bw.bytes(), bw.n, n)
    # a block of a stream cut short inside its payload: the block call fails with code 13, the next call succeeds
    rec = next(r for r in GOLDEN["streams"] if r["name"] == "len4097")
    d = _input(rec)
    hdr, hbits = _header(rec)
    p = hip.params("NONE", "CM", rec["block_size"])
    cap = hip.encode_bound(p, len(d))
    d_in, d_out, d_dec = hip.malloc(len(d) + 64), hip.malloc(cap), hip.malloc(len(d) + rec["block_size"] + 64)
    try:
        hip.h2d(d_in, d)
        bits = hip.encode_blocks(p, d_in, len(d), d_out, cap, prologue=hdr, prologue_bits=hbits)
        enc = bytearray(hip.d2h(d_out, (bits + 7) // 8))
        # the var-int of the block's only chunk (behind 5 + lw bits of length prefix, the mode byte and two length bytes): 3 bytes that
        # announce 2 MiB of payload, more than 32 bytes per byte of the 4,097
        written = 24 + cm_model.encode(d)[1]
        lw = (written >> 3).bit_length() - 1 + 4
        at = hbits + 5 + lw + 24
        for k in range(24):
            bit = (0xFFFF7F >> (23 - k)) & 1
            enc[(at + k) >> 3] = (enc[(at + k) >> 3] & ~(0x80 >> ((at + k) & 7))) | (bit * (0x80 >> ((at + k) & 7)))
        hip.h2d(d_out, bytes(enc))
        hipapi = importlib.import_module("kanzi_amd.hipapi")
        with pytest.raises(hipapi.KnzError) as e:
            hip.decode_blocks(p, d_out, bits, hbits, d_dec, len(d) + rec["block_size"])
        assert e.value.code == ERR_PROCESS_BLOCK
        hip.h2d(d_in, d)
        bits = hip.encode_blocks(p, d_in, len(d), d_out, cap, prologue=hdr, prologue_bits=hbits)
        ob, _, _ = hip.decode_blocks(p, d_out, bits, hbits, d_dec, len(d) + rec["block_size"])
        assert hip.d2h(d_dec, ob) == d
    finally:
        for ptr in (d_in, d_out, d_dec):
            hip.free(ptr)


def _host_cases():
    return [r for r in GOLDEN["streams"] if r["name"] in ("blocks_x32", "blocks_x64", "len2")] + GOLDEN["chains"] + GOLDEN["hosted"]


@pytest.mark.parametrize("rec", _host_cases(), ids=lambda r: r["name"])
def test_python_compressor_writes_and_reads_the_reference_file(tmp_path, rec):
    """kz.Compressor(..., entropy="CM") through the C API: the reference's .knz byte for byte (TEXT, in the variant CM selects, and UTF
    on the host in the last case), and kz.Decompressor reads it back. The C API's compressor is handed no input size, so the golden
    stream is the one the reference writes when it reads standard input (tools/make_cm_golden.py)."""
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    data = _input(rec)
    bs = rec["block_size"]
    path = str(tmp_path / "s.knz")
    c = kz.Compressor(path, rec["chain"], "CM", bs, 1, checksum=rec["checksum"])
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
    """kanzi_amd_cli -c -e CM: the reference's files, and -d reads them back."""
    cli = os.environ.get("KNZ_TEST_CLI", os.path.join(knzlib.PKG, "kanzi_amd_cli"))
    for rec in [r for r in _host_cases() if r["name"] in ("blocks_x32", "BWT+RANK+ZRLT", "LZP", "TEXT+UTF+BWT+LZP")]:
        data = _input(rec)
        src, out, back = str(tmp_path / "in.bin"), str(tmp_path / "out.knz"), str(tmp_path / "back.bin")
        open(src, "wb").write(data)
        extra = ["-x%d" % rec["checksum"]] if rec["checksum"] else []
        p = subprocess.run([cli, "-c", "-i", src, "-o", out, "-f", "-t", rec["chain"], "-e", "CM", "-b", str(rec["block_size"]), "-j", "1"] + extra,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        enc = open(out, "rb").read()
        assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"], rec["name"]
        p = subprocess.run([cli, "-d", "-i", out, "-o", back, "-f"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        assert open(back, "rb").read() == data


def test_cpp_cm_mirror():
    """CMPredictor / BinaryEntropyEncoder / BinaryEntropyDecoder of include/kanzi_amd.hpp: round trips directly, through the factories
    and the stream classes, and the refused constructor arguments, a predictor without a Context among them
    (tests/cpp/cm_mirror_test.cpp)."""
    exe = os.environ.get("KNZ_TEST_CM_MIRROR_EXE") or os.path.join(knzlib.ROOT, "tests", "cpp", "cm_mirror_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_second_tier_with_the_first_lowered(hip, monkeypatch):
    """No input of these tests exceeds the first tier of n + n / 8 bytes, so the paths behind it run here with KNZ_CM_TIER1_DIV=4, the
    library's debugging knob that makes the first tier n / 4 (first staging and knz_hip_encode_bound alike): blocks of random bytes
    are coded a second time into 32 n + 16 bytes, next to blocks of text that are not; an output buffer of the first tier is refused
    with code 12 and one of the second tier takes the reference's stream; the per-stage entry point, the sharded run encoder and the
    C++ mirror (entropy encoder and stream classes, tests/cpp/cm_mirror_test.cpp) retry by themselves."""
    monkeypatch.setenv("KNZ_CM_TIER1_DIV", "4")
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    # per stage: the kernel runs twice, the entry point retries with the second tier
    data = cm_cases.make(cm_cases.VARINT[2])                 # 17,000 random bytes: above the lowered bound and its fixed slack
    assert hip.encode_bound(hip.params("NONE", "CM", 1 << 20), len(data)) < len(data)
    hip.set_profiling(True)
    try:
        got, gbits = hip.entropy_encode("CM", data)
        launches = sum(k[2] for k in hip.kernel_times() if k[0] == "k_cm_encode")
    finally:
        hip.set_profiling(False)
    assert (got, gbits) == cm_model.encode(data) and launches >= 2
    # one block above the lowered bound; several blocks of which some are marked (skewed bytes) and some not (constant bytes)
    for name in ("varint3", "blocks_x64"):
        rec = next(r for r in GOLDEN["streams"] if r["name"] == name)
        d = _input(rec)
        bs = rec["block_size"]
        hdr, hbits = _header(rec)
        p = hip.params("NONE", "CM", bs, checksum=rec["checksum"])
        cap = hip.encode_bound(p, len(d))
        cap2 = cap + 32 * len(d)
        d_in, d_out, d_dec = hip.malloc(len(d) + 64), hip.malloc(cap2), hip.malloc(len(d) + bs + 64)
        try:
            hip.h2d(d_in, d)
            if name == "varint3":
                assert cap < rec["knz_len"]
                with pytest.raises(hipapi.KnzError) as e:
                    hip.encode_blocks(p, d_in, len(d), d_out, cap, prologue=hdr, prologue_bits=hbits)
                assert e.value.code == 12
            bits = hip.encode_blocks(p, d_in, len(d), d_out, cap2, prologue=hdr, prologue_bits=hbits)
            enc = hip.d2h(d_out, (bits + 7) // 8)
            assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]
            ob, _, _ = hip.decode_blocks(p, d_out, bits, hbits, d_dec, len(d) + bs)
            assert hip.d2h(d_dec, ob) == d
        finally:
            for ptr in (d_in, d_out, d_dec):
                hip.free(ptr)
    # the sharded run encoder
    sharded = importlib.import_module("kanzi_amd.sharded")
    rec = next(r for r in GOLDEN["streams"] if r["name"] == "varint3")
    d = _input(rec)
    enc, bits = sharded.DeviceRunEncoder(0, "NONE", "CM", rec["block_size"], orig_size=rec["orig_size"])(d, 0, True, True)
    assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]
    # the C++ mirror: DeviceEntropyEncoder::encode and CompressedOutputStream on random bytes
    exe = os.environ.get("KNZ_TEST_CM_MIRROR_EXE") or os.path.join(knzlib.ROOT, "tests", "cpp", "cm_mirror_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, KNZ_CM_TIER1_DIV="4"))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
