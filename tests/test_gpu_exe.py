"""EXE (EXECodec, transform id 9) on the device: per stage through the C ABI, in whole chains through knz_hip_encode_blocks /
knz_hip_decode_blocks, in a .knz file with TEXT on the host in front, through the C++ mirror and through the command-line tool.
Expected results come from tests/golden/exe.json (written from the reference by tools/make_exe_golden.py)."""
import hashlib
import importlib
import json
import os
import subprocess

import pytest

import exe_cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exe.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def _input(rec):
    d = exe_cases.make(rec["recipe"])
    assert md5(d) == rec["input_md5"], rec["recipe"]
    return d


@pytest.fixture(scope="module")
def forward_outputs(hip):
    """The device's forward result of every stage record by name, computed once: (input, ok, bytes, data type left)."""
    out = {}
    for rec in GOLDEN["stage"]:
        d = _input(rec)
        out[rec["name"]] = (d,) + tuple(hip.transform_forward_dt("EXE", d, rec["cap"], rec["dtype"]))
    return out


def test_stage_forward_golden_and_round_trip(hip, forward_outputs):
    """x86 and ARM64 code found by the heuristics at 4,095 (refused) to 300,001 bytes and in one block of 1.7 MB (more chunks than one
    step of the per-block composition); ELF 32 / 64 in both byte orders, PE and Mach-O headers, an unknown architecture, a rejected
    header, a header that fails after it moved the range, a code range too short for 16 matches; preset types; random bytes, text and
    ACGT; the three exits at the end of the code, the ff000000 escape, 9b bytes, 0f runs, a jump across a chunk border, growth on both
    sides of the 2 % cap; ARM64 targets below 0 up to the count a block affords and beyond; code that starts off a multiple of 4.
    The inverse gives what the reference's inverse gives (the input, except where the reference loses it too), into a destination
    of the input's length, which is smaller than the encoded block."""
    for rec in GOLDEN["stage"]:
        d, ok, fwd, dt = forward_outputs[rec["name"]]
        assert int(ok) == rec["ok"], ("ok", rec["name"])
        assert dt == rec["dtype_out"], ("data type", rec["name"])
        if not rec["ok"]:
            continue
        assert len(fwd) == rec["fwd_len"] and md5(fwd) == rec["fwd_md5"], ("forward", rec["name"])
        ok, back = hip.transform_inverse("EXE", fwd, len(d))
        assert ok and md5(back) == rec["inv_md5"] and (back == d) == bool(rec["lossless"]), ("round trip", rec["name"])


def test_stage_without_a_context_starts_undefined(hip, forward_outputs):
    """knz_hip_transform_forward has no Context: a fresh UNDEFINED one per block, so no type keeps a block from the detection."""
    for name in ("x86 8192", "arm 4096", "elf64 x86"):
        d, ok, fwd, _ = forward_outputs[name]
        assert ok and (ok, fwd) == hip.transform_forward("EXE", d, exe_cases.max_encoded(len(d)))
    ok, _ = hip.transform_forward("EXE", forward_outputs["text"][0], exe_cases.max_encoded(8192))
    assert not ok


def test_stage_refuses_short_destination(hip, forward_outputs):
    """EXECodec.cpp:77: a destination one byte below getMaxEncodedLength is refused and the type stays, the bound itself is enough."""
    d = forward_outputs["x86 8192"][0]
    ok, _, dt = hip.transform_forward_dt("EXE", d, exe_cases.max_encoded(len(d)) - 1, 0)
    assert not ok and dt == 0
    ok, _, dt = hip.transform_forward_dt("EXE", d, exe_cases.max_encoded(len(d)), 0)
    assert ok and dt == exe_cases.EXE


def test_stage_inverse_of_cut_and_damaged_input(hip, forward_outputs):
    """Outputs of the x86 and the ARM64 path, with and without bytes in front of the code, whole; cut inside the header, the copied
    prefix and the code and 1 to 4 bytes before its end; with the end of the code moved by one and behind the block, its start negative
    and behind the code; another mode byte; an escape as the last byte of the code; an ARM64 escape pair cut in half: the reference's
    verdict at both capacities, and its bytes where it accepts."""
    n_refused = 0
    for rec in GOLDEN["damaged"]:
        bad = exe_cases.damage(forward_outputs[rec["stage"]][2], rec["op"])
        assert md5(bad) == rec["input_md5"], (rec["stage"], rec["op"])
        ok, inv = hip.transform_inverse("EXE", bad, rec["cap"])
        assert int(ok) == rec["ok"], ("ok", rec["stage"], rec["op"], rec["cap"])
        n_refused += 0 if ok else 1
        if rec["ok"]:
            assert len(inv) == rec["inv_len"] and md5(inv) == rec["inv_md5"], ("inverse", rec["stage"], rec["op"], rec["cap"])
    assert n_refused > 0


def _stream(hip, chain, entropy, bs, checksum, data, rec, n_blocks):
    """The stream equals the reference's; it decodes back in one call and as runs of 1, 2 and 3 blocks."""
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
            assert nb == n_blocks and hip.d2h(d_dec, ob) == data, chain
            out, start, done, step = bytearray(), 0, 0, 1
            while done < n_blocks:
                ob, start, k = hip.decode_blocks(p, d_out, bits, start, d_dec, len(data) + bs, max_blocks=step)
                assert k > 0
                out += hip.d2h(d_dec, ob)
                done += k
                step = step % 3 + 1
            assert bytes(out) == data, chain
        finally:
            hip.free(d_dec)
    finally:
        hip.free(d_in)
        hip.free(d_out)


def test_ragged_batch_bit_exact_and_decodes(hip):
    """71 blocks of 4,096 bytes (the last one 100) in one batch: x86, ARM64, text, random bytes and ACGT in turn."""
    rec = GOLDEN["ragged"]
    data = exe_cases.make(exe_cases.RAGGED)
    assert md5(data) == rec["input_md5"]
    _stream(hip, "EXE", "NONE", rec["block_size"], 0, data, rec, 71)


@pytest.mark.parametrize("idx", range(len(exe_cases.STREAM_CHAINS)))
def test_chain_bit_exact_and_decodes(hip, idx):
    """64 KiB blocks of x86, text, ARM64, an ELF block (its type preset from the magic), x86 again and a tail of 1,000 bytes through
    EXE / NONE, EXE+RLT / HUFFMAN, EXE+ROLZX / ANS0 (the type EXE writes reaches ROLZX), EXE+PACK+ZRLT / FPAQ (PACK refuses the EXE
    blocks) and EXE+BWT+RANK+ZRLT / ANS0 with checksums."""
    rec = GOLDEN["streams"][idx]
    data = exe_cases.make(exe_cases.STREAM)
    assert md5(data) == rec["input_md5"]
    _stream(hip, rec["chain"], rec["entropy"], rec["block_size"], rec["checksum"], data, rec, exe_cases.STREAM_BLOCKS)


@pytest.mark.parametrize("idx", range(len(GOLDEN["hosted"])))
def test_hosted_chain_bit_exact_and_decodes(tmp_path, idx):
    """TEXT on the host in front of EXE and RLT on the device, at 1 and 3 jobs: TEXT takes the text blocks and EXE refuses them by their
    type, TEXT refuses the code blocks and EXE takes them. The .knz equals the reference's and decodes back."""
    import knzlib
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    rec = GOLDEN["hosted"][idx]
    data = exe_cases.make(exe_cases.STREAM)
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


def test_cpp_exe_mirror():
    """EXECodec of include/kanzi_amd.hpp: the constructors, getMaxEncodedLength, the data type written back, round trips directly,
    through TransformFactory and through the stream classes (tests/cpp/exe_mirror_test.cpp)."""
    import knzlib
    exe = os.path.join(knzlib.ROOT, "tests", "cpp", "exe_mirror_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_cli_reads_and_writes_what_the_reference_does(tmp_path):
    """kanzi_amd_cli -c -t EXE+RLT -e HUFFMAN on about 300 KB: byte-identical to the reference tool's file, each tool reads the other's."""
    import knzlib
    ref_cli = os.path.join(knzlib.ROOT, "oracle", "_ref", "kanzi")
    if not os.path.exists(ref_cli):
        pytest.skip("the reference's command-line tool is not built (oracle/_ref/kanzi)")
    cli = os.path.join(knzlib.PKG, "kanzi_amd_cli")
    assert os.path.exists(cli), "run __graft_entry__.build()"
    data = _input(GOLDEN["cli"])
    src, ours, theirs, back = (str(tmp_path / n) for n in ("in.bin", "ours.knz", "theirs.knz", "back.bin"))
    open(src, "wb").write(data)
    args = exe_cases.CLI_ARGS + ["-b", "65536", "-j", "1"]
    p = subprocess.run([cli, "-c", "-i", src, "-o", ours, "-f"] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    p = subprocess.run([ref_cli, "-c", "-i", src, "-o", theirs, "-f"] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert open(ours, "rb").read() == open(theirs, "rb").read()
    assert len(open(ours, "rb").read()) != len(data)
    p = subprocess.run([ref_cli, "-d", "-i", ours, "-o", back, "-f", "-j", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and open(back, "rb").read() == data, p.stderr
    os.remove(back)
    p = subprocess.run([cli, "-d", "-i", theirs, "-o", back, "-f"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and open(back, "rb").read() == data, p.stderr
