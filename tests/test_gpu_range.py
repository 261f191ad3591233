"""RANGE (entropy id 4) on the device: per stage through the C ABI against tests/range_model.py (pinned to the reference by
tests/test_range_model.py), whole streams against the reference's digests in tests/golden/range.json (tools/make_range_golden.py), the
decoder's divide against integer division, refusals of damaged streams, and the host interfaces."""
import hashlib
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import knzlib
import range_cases
import range_model

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "range.json")))
ERR_PROCESS_BLOCK = 13          # what the ANS0 decoder returns for a bad table or a short payload


def md5(b):
    return hashlib.md5(b).hexdigest()


def _input(rec):
    d = range_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["name"]
    return d


def _header(rec, chain="NONE"):
    knzlib.load_pkg()
    framing = importlib.import_module("kanzi_amd.framing")
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    hdr, bits = framing.make_header(4, hipapi.transform_type(chain), rec["block_size"], rec["checksum"], rec["orig_size"])
    assert bits == rec["header_bits"]
    return hdr, bits


_model_cache = {}


def _model(name, data):
    """(bytes, bits, Stats) of the model for one block, computed once."""
    if name not in _model_cache:
        st = range_model.Stats()
        enc, bits = range_model.encode(data, st)
        _model_cache[name] = (enc, bits, st)
    return _model_cache[name]


STAGE = [(n, r) for n, r, bs, ck in range_cases.STREAMS if bs == 1 << 20]


@pytest.mark.parametrize("name,recipe", STAGE, ids=[n for n, _ in STAGE])
def test_stage_encode_matches_model_and_decodes(hip, name, recipe):
    """knz_hip_entropy_encode / _decode: lengths 1 to 3 x 32,768 + 5 (log ranges 8 to 12, a short last chunk), alphabets of 1, 2, 63,
    64, 65 and 256 symbols (groups of 6 and 8), a skewed one, n == scale, a constant chunk between two coded ones, the underflow
    branch, the chunk with the most units: the bits are the model's, and they decode back with every bit used."""
    data = range_cases.make(recipe)
    enc, bits, st = _model(name, data)
    got, gbits = hip.entropy_encode("RANGE", data)
    assert gbits == bits and got == enc
    n, back, used = hip.entropy_decode("RANGE", got, len(data), in_bits=gbits)
    assert n == len(data) and back == data and used == bits
    for u in st.units:
        assert u <= 32768 + 32768 // 64 + 2          # the bound the staging region is sized by (range.hip)


def test_branches_the_cases_are_there_for():
    """The model's counters say that the inputs take the branches they were chosen for."""
    _, _, st = _model("underflow", range_cases.make(range_cases.UNDERFLOW))
    assert st.underflows >= 1
    # the chunk of the cases that leaves the most units: full-alphabet random bytes, 8 bits a byte, well inside the derived bound
    most = max(max(_model(n, range_cases.make(r))[2].units or [0]) for n, r in STAGE)
    assert most == max(max(_model(n, range_cases.make(dict(STAGE)[n]))[2].units) for n in ("uniform256", "middle_constant", "underflow"))
    assert 8 * 32768 // 28 - 16 <= most <= 32768 + 32768 // 64 + 2
    _, _, st = _model("middle_constant", range_cases.make(dict(STAGE)["middle_constant"]))
    assert len(st.units) == 2                        # three chunks, the middle one without payload


def test_decode_from_a_bit_offset(hip):
    data = range_cases.make(["text", 70000, 4])
    enc, bits, _ = _model("text", data)
    for lead in (3, 13):
        shifted = ((((1 << lead) - 1) << (8 * len(enc))) | int.from_bytes(enc, "big"))
        nbytes = (lead + 8 * len(enc) + 7) // 8
        shifted = (shifted << (8 * nbytes - lead - 8 * len(enc))).to_bytes(nbytes, "big")
        n, back, used = hip.entropy_decode("RANGE", shifted, len(data), start_bit=lead, in_bits=lead + bits)
        assert n == len(data) and back == data and used == bits


def test_divide_is_exact(hip):
    """The decoder's reciprocal-based divide against integer division: more than 10^6 (code - low, range >> lr) pairs recorded from
    model decodes, and the extremes -- the smallest and largest range after each shift, quotients 0, 1 and 2^lr - 1, remainders 0
    and r - 1."""
    d, r = [], []
    runs = [(n, range_cases.make(rc)) for n, rc in STAGE]
    runs.append(("top_up", range_cases.make(["alpha", 10 ** 6 + 40000 - sum(len(b) for _, b in runs if len(set(b)) > 1), 5, 256])))
    for name, data in runs:
        enc, bits, _ = _model(name, data)
        st = range_model.Stats()
        range_model.decode(enc, len(data), 0, bits, st)
        d += [p[0] for p in st.pairs]
        r += [p[1] for p in st.pairs]
    assert len(d) >= 10 ** 6
    for lr in range(8, 16):
        lo, hi = 0x10000 >> lr, ((1 << 60) - 1) >> lr
        for rr in (lo, lo + 1, hi - 1, hi, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 32) - 1, (1 << 32) + 1, (1 << 52) - 1):
            if not lo <= rr <= hi:
                continue
            for q in (0, 1, 2, (1 << lr) - 2, (1 << lr) - 1, 1 << (lr - 1)):
                for rem in (0, 1, rr // 2, rr - 1):
                    d.append(q * rr + rem)
                    r.append(rr)
    d, r = np.array(d, dtype=np.uint64), np.array(r, dtype=np.uint64)
    q = hip.range_divide(d, r)
    want = (d // r).astype(np.uint32)
    assert np.array_equal(q, want), int(np.flatnonzero(q != want)[0])


@pytest.mark.parametrize("kind,idx", [(k, i) for k in ("streams", "chains") for i in range(len(GOLDEN[k]))],
                         ids=[r["name"] for k in ("streams", "chains") for r in GOLDEN[k]])
def test_stream_is_the_references_and_decodes(hip, kind, idx):
    """knz_hip_encode_blocks behind the stream header writes the reference's bytes (one block and several of different lengths,
    checksums 32 and 64, copy blocks, BWT+MTFT+ZRLT and RLT in front -- RLT picks its escape by the entropy id); knz_hip_decode_blocks
    gives the input back, also from the non-zero start bit behind the header."""
    rec = GOLDEN[kind][idx]
    data = _input(rec)
    bs = rec["block_size"]
    hdr, hbits = _header(rec, rec["chain"])
    p = hip.params(rec["chain"], "RANGE", bs, checksum=rec["checksum"])
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


def _bad_then_good(hip, stream, bits, count):
    n, _, used = hip.entropy_decode("RANGE", stream, count, in_bits=bits)
    assert n == -1 and used <= bits
    good = range_cases.make(["geom", 1024, 105, 30])
    enc, gbits = range_model.encode(good)
    n, back, _ = hip.entropy_decode("RANGE", enc, len(good), in_bits=gbits)
    assert n == len(good) and back == good


def test_refusals_leave_the_context_healthy(hip):
    """A frequency width above the log range, frequencies that sum to the scale, a payload cut at several bit positions: refused (the
    per-stage call reports -1, the block call the ANS0 decoder's code), and a good block decodes right after."""
    for freqs, width in (([100, 200], 13), ([2048, 2048], 12)):
        bw = range_model.BitWriter()
        range_model.put_alphabet(bw, [0, 1, 2])
        bw.put(4, 3)
        bw.put(width, 4)
        for f in freqs:
            bw.put(f - 1, width)
        bw.put(0, 200)
        _bad_then_good(hip, bw.bytes(), bw.n, 5000)
    data = range_cases.make(["geom", 4097, 108, 30])
    enc, bits = range_model.encode(data)
    for cut in (1, 9, 100, bits // 2, bits - 61, bits - 28, bits - 1):
        _bad_then_good(hip, enc[:(cut + 7) // 8], cut, len(data))
    # a block of a stream whose payload is damaged: the block call fails with the code of a bad ANS0 table
    rec = next(r for r in GOLDEN["streams"] if r["name"] == "len4097")
    d = _input(rec)
    hdr, hbits = _header(rec)
    p = hip.params("NONE", "RANGE", rec["block_size"])
    cap = hip.encode_bound(p, len(d))
    d_in, d_out, d_dec = hip.malloc(len(d) + 64), hip.malloc(cap), hip.malloc(len(d) + rec["block_size"] + 64)
    try:
        hip.h2d(d_in, d)
        bits = hip.encode_blocks(p, d_in, len(d), d_out, cap, prologue=hdr, prologue_bits=hbits)
        enc = bytearray(hip.d2h(d_out, (bits + 7) // 8))
        # the first frequency width field (behind 5 + lw bits of length prefix, mode byte, two length bytes, the partial alphabet and
        # 3 bits of log range): set to 15
        alphabet = sorted(set(d))
        assert 1 < len(alphabet) < 256
        written = 24 + range_model.encode(d)[1]
        lw = (written >> 3).bit_length() - 1 + 4
        at = hbits + 5 + lw + 24 + 6 + 8 * ((alphabet[-1] >> 3) + 1) + 3
        for k in range(4):
            enc[(at + k) >> 3] |= 0x80 >> ((at + k) & 7)
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
    return ([r for r in GOLDEN["streams"] if r["name"] in ("blocks", "blocks_x32", "blocks_x64", "middle_constant", "copy_block")]
            + GOLDEN["chains"] + GOLDEN["hosted"])


@pytest.mark.parametrize("rec", _host_cases(), ids=lambda r: r["name"])
def test_python_compressor_writes_and_reads_the_reference_file(tmp_path, rec):
    """kz.Compressor(..., entropy="RANGE") through the C API: the reference's .knz byte for byte (TEXT and UTF on the host in the last
    case), and kz.Decompressor reads it back. The C API's compressor is handed an empty file and no input size, so like the
    reference's it writes a header without the original size: the golden stream is the one the reference writes when it reads
    standard input, which differs from the sized one in the header alone (tools/make_range_golden.py asserts that)."""
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    data = _input(rec)
    bs = rec["block_size"]
    path = str(tmp_path / "s.knz")
    c = kz.Compressor(path, rec["chain"], "RANGE", bs, 1, checksum=rec["checksum"])
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
    """kanzi_amd_cli -c -e RANGE: the reference's files, and -d reads them back."""
    cli = os.environ.get("KNZ_TEST_CLI", os.path.join(knzlib.PKG, "kanzi_amd_cli"))
    for rec in [r for r in _host_cases() if r["name"] in ("blocks_x32", "RLT", "TEXT+UTF+BWT+RANK+ZRLT")]:
        data = _input(rec)
        src, out, back = str(tmp_path / "in.bin"), str(tmp_path / "out.knz"), str(tmp_path / "back.bin")
        open(src, "wb").write(data)
        extra = ["-x%d" % rec["checksum"]] if rec["checksum"] else []
        p = subprocess.run([cli, "-c", "-i", src, "-o", out, "-f", "-t", rec["chain"], "-e", "RANGE", "-b", str(rec["block_size"]), "-j", "1"] + extra,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        enc = open(out, "rb").read()
        assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"], rec["name"]
        p = subprocess.run([cli, "-d", "-i", out, "-o", back, "-f"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        assert open(back, "rb").read() == data


def test_cpp_range_mirror():
    """RangeEncoder / RangeDecoder of include/kanzi_amd.hpp: round trips directly, through the factories and the stream classes, and the
    refused constructor arguments (tests/cpp/range_mirror_test.cpp)."""
    exe = os.environ.get("KNZ_TEST_RANGE_MIRROR_EXE") or os.path.join(knzlib.ROOT, "tests", "cpp", "range_mirror_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_wide_frequency_chunks_are_the_references(hip):
    """A short chunk with a nearly full alphabet on which the reference's normalisation wraps a frequency below zero (range_cases.WIDE;
    found by tools/gpu_soak.py): the reference writes a chunk that it cannot read, and the device writes the same bits -- per stage, and
    inside framed streams whose block headers (checksums of 0, 32 and 64 bits) put the chunk at different positions of the block's
    64-bit words -- and refuses to read them as the reference does."""
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    for rec in GOLDEN["wide"]["stage"]:
        d = _input(dict(rec, name=str(rec["recipe"])))
        enc, bits = hip.entropy_encode("RANGE", d)
        assert bits == rec["bits"] and md5(enc) == rec["enc_md5"], rec["recipe"]
        assert not rec["ref_decodes"]
        try:
            dec, out, _ = hip.entropy_decode("RANGE", enc, len(d))
            assert not (dec == len(d) and out == d), rec["recipe"]
        except hipapi.KnzError:
            pass
    for rec in GOLDEN["wide"]["streams"]:
        d = _input(dict(rec, name=str(rec["recipe"])))
        bs = rec["block_size"]
        p = hip.params("NONE", "RANGE", bs, rec["checksum"], jobs=rec["jobs"])
        cap = hip.encode_bound(p, len(d)) + 64
        d_in, d_out, d_dec = hip.malloc(len(d) + 64), hip.malloc(cap), hip.malloc(len(d) + 2 * bs + 64)
        try:
            hip.h2d(d_in, d)
            bits = hip.encode_blocks(p, d_in, len(d), d_out, cap)
            enc = hip.d2h(d_out, (bits + 7) // 8)
            assert len(enc) == rec["stream_len"] and md5(enc) == rec["stream_md5"], rec["recipe"]
            assert not rec["ref_decodes"]
            with pytest.raises(hipapi.KnzError):
                hip.decode_blocks(p, d_out, bits, 0, d_dec, len(d) + bs)
        finally:
            hip.free(d_in)
            hip.free(d_out)
            hip.free(d_dec)
    # the context is still usable
    d = range_cases.make(["text", 70000, 4])
    enc, bits = hip.entropy_encode("RANGE", d)
    dec, out, used = hip.entropy_decode("RANGE", enc, len(d))
    assert dec == len(d) and out == d and used == bits
