"""TEXT (TextCodec, transform id 10) on the device: per stage through the C ABI in both encodings and three map sizes, in whole chains
through knz_hip_encode_blocks / knz_hip_decode_blocks, and in .knz files through the stream classes. Expected results come from
tests/golden/text.json (tools/make_text_golden.py)."""
import hashlib
import importlib
import json
import os
import subprocess
import sys

import pytest

import text_cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text.json")))
COMBOS = [(codec, bs) for codec in (1, 2, 3) for bs in text_cases.BLOCK_SIZES]


def md5(b):
    return hashlib.md5(b).hexdigest()


@pytest.fixture(scope="module")
def blocks():
    """The inputs of the stage records by name, built once"""
    out = {}
    for r in GOLDEN["stage"]:
        if r["name"] not in out:
            out[r["name"]] = text_cases.make(r["recipe"])
            assert md5(out[r["name"]]) == r["input_md5"], r["name"]
    return out


def test_text_is_a_device_stage(hip):
    assert hip.L.knz_hip_transform_supported(10) == 1


@pytest.mark.parametrize("codec,bs", COMBOS)
def test_stage_forward_golden_and_round_trip(hip, blocks, codec, bs):
    """Every stage record of one codec and one stream block size (hash maps of 2^13, 2^14, 2^17 and 2^19 / 2^20 slots): blocks of 1,023
    (refused) and 1,024 bytes, plain text, leading spaces, CRLF with and without a bare LF, XML, escape bytes, high bytes on both sides of a
    quarter, a magic number, every preset type, every non-text verdict, words of 2, 3, 31 and 32 letters, static words and their case
    flips, a new word twice in a window, words that share a slot inside a window and across windows, a dictionary that grows, one that
    passes 16,384 entries and then meets new three-letter words, one that wraps at 2^19 entries (4 MiB), and a block refused midway.
    The verdict, the data type left and the bytes are the recorded ones; the inverse gives the input back into a destination of its length."""
    entropy = text_cases.ENTROPY[codec]
    recs = [r for r in GOLDEN["stage"] if r["codec"] == codec and r["block_size"] == bs]
    assert len(recs) == len(text_cases.stage_cases())
    for r in recs:
        d = blocks[r["name"]]
        ok, fwd, dt = hip.transform_forward_bs("TEXT", d, len(d), r["dtype"], entropy, bs)
        assert int(ok) == r["ok"], ("ok", r["name"])
        assert dt == r["dtype_out"], ("data type", r["name"])
        if not r["ok"]:
            continue
        assert len(fwd) == r["fwd_len"] and md5(fwd) == r["fwd_md5"], ("forward", r["name"])
        ok, back = hip.transform_inverse_bs("TEXT", fwd, len(d), entropy, bs)
        assert ok and back == d, ("round trip", r["name"])


def test_stage_entry_points_without_a_block_size(hip, blocks):
    """knz_hip_transform_forward / _forward_dt / _inverse take TEXT with block size 0; the inverse without an entropy id reads codec 1."""
    d = blocks["plain 9000"]
    rec = [r for r in GOLDEN["stage"] if r["name"] == "plain 9000" and r["block_size"] == 0]
    for r in rec:
        ok, fwd = hip.transform_forward("TEXT", d, len(d), text_cases.ENTROPY[r["codec"]])
        assert ok and md5(fwd) == r["fwd_md5"]
        ok, fwd2, dt = hip.transform_forward_dt("TEXT", d, len(d), 0, text_cases.ENTROPY[r["codec"]])
        assert ok and fwd2 == fwd and dt == 1
    ok, fwd = hip.transform_forward("TEXT", d, len(d))
    assert ok and md5(fwd) == rec[0]["fwd_md5"]
    ok, back = hip.transform_inverse("TEXT", fwd, len(d))
    assert ok and back == d
    ok, _ = hip.transform_forward("TEXT", d, len(d) - 1)
    assert not ok, "a destination below the block's length is refused"


def test_stage_inverse_of_damaged_input(hip, blocks):
    """A block cut inside an index, an index at or beyond the dictionary size, index 0 of codec 2 in two and three bytes, an entry no
    word has taken, and a destination too short: the host code's verdict, and its bytes where it accepts."""
    n_refused = 0
    d = blocks[text_cases.DAMAGE_FROM]
    for codec in (1, 2, 3):
        entropy = text_cases.ENTROPY[codec]
        ok, fwd, _ = hip.transform_forward_bs("TEXT", d, len(d), 0, entropy, 0)
        assert ok
        for r in [r for r in GOLDEN["damaged"] if r["codec"] == codec]:
            bad = text_cases.damage(fwd, r["op"], codec)
            assert md5(bad) == r["input_md5"], r["name"]
            ok, inv = hip.transform_inverse_bs("TEXT", bad, r["cap"], entropy, 0)
            assert int(ok) == r["ok"], (r["name"], codec)
            n_refused += 0 if ok else 1
            if r["ok"]:
                assert len(inv) == r["inv_len"] and md5(inv) == r["inv_md5"], (r["name"], codec)
    assert n_refused >= 12


def _stream(hip, data, rec, n_blocks, runs=True):
    """The stream equals the reference's; it decodes back in one call and (runs) as runs of 1, 2 and 3 blocks."""
    chain, bs = rec["chain"], rec["block_size"]
    p = hip.params(chain, rec["entropy"], bs, checksum=rec["checksum"])
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
            while runs and done < n_blocks:
                ob, start, k = hip.decode_blocks(p, d_out, bits, start, d_dec, len(data) + bs, max_blocks=step)
                assert k > 0
                out += hip.d2h(d_dec, ob)
                done += k
                step = step % 3 + 1
            assert bytes(out) == data or not runs, chain
        finally:
            hip.free(d_dec)
    finally:
        hip.free(d_in)
        hip.free(d_out)


@pytest.mark.parametrize("idx", range(len(text_cases.MIXED_CHAINS)))
def test_mixed_batch_bit_exact_and_decodes(hip, idx):
    """Eight blocks of 64 KiB in one batch: text, CRLF text, XML, ACGT, all byte values, UTF-8, text with escape bytes and distinct
    words, in both encodings."""
    rec = GOLDEN["mixed"][idx]
    data = text_cases.mixed()
    assert md5(data) == rec["input_md5"]
    _stream(hip, data, rec, len(text_cases.MIXED_KINDS))


@pytest.mark.parametrize("idx", range(len(text_cases.STREAM_CHAINS)))
def test_chain_bit_exact_and_decodes(hip, idx):
    """300,000 bytes of text in blocks of 64 KiB against the reference's streams: the presets of levels 5 to 9, TEXT behind each of
    ZRLT, PACK, MM, UTF, ROLZX, EXE and RLT, and TEXT+RLT."""
    rec = GOLDEN["streams"][idx]
    data = text_cases.make(text_cases.STREAM)
    assert md5(data) == rec["input_md5"]
    _stream(hip, data, rec, text_cases.STREAM_BLOCKS)


def test_lzx_behind_text_is_refused(hip):
    """TEXT sets the data type, which the device LZ stages do not read: refused like LZ / LZX behind PACK."""
    p = hip.params("TEXT+LZX", "NONE", 65536)
    d_in, d_out = hip.malloc(4096), hip.malloc(65536)
    try:
        with pytest.raises(Exception) as e:
            hip.encode_blocks(p, d_in, 2048, d_out, 65536)
        assert e.value.code == 3 and "LZ / LZX behind" in str(e.value), "KNZ_ERR_INVALID_CODEC"
    finally:
        hip.free(d_in)
        hip.free(d_out)


def _knz(kz, path, chain, entropy, bs, jobs, data):
    c = kz.Compressor(path, chain, entropy, bs, jobs)
    for off in range(0, len(data), bs):
        c.compress(data[off:off + bs])
    c.close()
    enc = open(path, "rb").read()
    d = kz.Decompressor(path, buffer_size=bs, jobs=jobs)
    out = bytearray()
    while True:
        chunk = d.decompress(bs)
        out += chunk
        if len(chunk) < bs:
            break
    d.close()
    assert bytes(out) == data, (chain, jobs)
    return enc


CHILD = """
import importlib, sys
sys.path.insert(0, %r)
import knzlib, text_cases
knzlib.load_pkg()
kz = importlib.import_module("kanzi_amd.kanzi")
data = text_cases.make(text_cases.STREAM)
c = kz.Compressor(sys.argv[1], sys.argv[2], sys.argv[3], 65536, int(sys.argv[4]))
for off in range(0, len(data), 65536):
    c.compress(data[off:off + 65536])
c.close()
"""


@pytest.mark.parametrize("jobs", (1, 3))
def test_knz_files_through_the_stream_classes(tmp_path, jobs):
    """The level 5 and level 7 chains through kz.Compressor / kz.Decompressor: TEXT in front and TEXT behind LZP, batched on the device.
    They decode back, and with KNZ_HOST_TEXT=1 in a child process (TEXT on the host, the path of before) the level 5 file is the same."""
    import knzlib
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    data = text_cases.make(text_cases.STREAM)
    lead = _knz(kz, str(tmp_path / "a.knz"), "TEXT+UTF+BWT+RANK+ZRLT", "ANS0", 65536, jobs, data)
    _knz(kz, str(tmp_path / "b.knz"), "LZP+TEXT+UTF+BWT+LZP", "CM", 65536, jobs, data)
    other = str(tmp_path / "c.knz")
    r = subprocess.run([sys.executable, "-c", CHILD % os.path.dirname(os.path.abspath(__file__)), other, "TEXT+UTF+BWT+RANK+ZRLT", "ANS0", str(jobs)],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, KNZ_HOST_TEXT="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(other, "rb").read() == lead


@pytest.mark.parametrize("idx", range(len(text_cases.CLI_LEVELS)))
def test_cli_level_writes_the_reference_file(tmp_path, idx):
    """kanzi_amd_cli -c -l 7, -l 8 and -l 9 with -b 64k on 300,000 bytes of text: byte-identical to what the reference's tool writes (recorded), and back to
    the input."""
    import knzlib
    cli = os.path.join(knzlib.PKG, "kanzi_amd_cli")
    assert os.path.exists(cli), "run __graft_entry__.build()"
    rec = GOLDEN["cli"][idx]
    data = text_cases.make(text_cases.STREAM)
    assert md5(data) == rec["input_md5"]
    src, out, back = (str(tmp_path / n) for n in ("in.txt", "out.knz", "back.txt"))
    open(src, "wb").write(data)
    p = subprocess.run([cli, "-c", "-i", src, "-o", out, "-f", "-j", "1", "-l", str(rec["level"]), "-b", "64k"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    enc = open(out, "rb").read()
    assert len(enc) == rec["knz_len"] and md5(enc) == rec["knz_md5"]
    p = subprocess.run([cli, "-d", "-i", out, "-o", back, "-f"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and open(back, "rb").read() == data, p.stderr


def test_cli_level_2_stays_refused(tmp_path):
    """Level 2 (DNA+LZ: LZ behind a stage that sets the data type) is refused with a message, nothing written."""
    import knzlib
    cli = os.path.join(knzlib.PKG, "kanzi_amd_cli")
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.knz")
    open(src, "wb").write(text_cases.make(["plain", 5000, 1]))
    p = subprocess.run([cli, "-c", "-i", src, "-o", out, "-f", "-l", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "level" in p.stderr and not os.path.exists(out)


@pytest.mark.parametrize("idx", range(len(text_cases.DNA_CHAINS)))
def test_dna_chain_bit_exact_and_decodes(hip, idx):
    """DNA (id 19, PACK that takes DNA blocks only) in front of RLT and alone, on an ACGT block (taken) and a text block (refused)."""
    rec = GOLDEN["dna"][idx]
    data = text_cases.dna_blocks()
    assert md5(data) == rec["input_md5"]
    _stream(hip, data, rec, len(text_cases.DNA_KINDS))


def test_dna_stage_refusals(hip):
    """AliasCodec.cpp:66 and :93: a preset type other than UNDEFINED or DNA is refused and stays; a block whose detection does not say
    DNA is refused after the type it found was written; PACK takes the same text block."""
    acgt, text = text_cases.make(text_cases.DNA_KINDS[0]), text_cases.make(["small", 3000, 14])
    ok, fwd, dt = hip.transform_forward_dt("DNA", acgt, len(acgt) + 1024, 0)
    assert ok and dt == 6 and len(fwd) < len(acgt) * 3 // 4
    assert (ok, fwd, dt) == tuple(hip.transform_forward_dt("PACK", acgt, len(acgt) + 1024, 0))
    assert hip.transform_inverse("DNA", fwd, len(acgt)) == (1, acgt)
    ok, _, dt = hip.transform_forward_dt("DNA", acgt, len(acgt) + 1024, 6)
    assert ok and dt == 6
    ok, _, dt = hip.transform_forward_dt("DNA", acgt, len(acgt) + 1024, 1)
    assert not ok and dt == 1
    ok, _, dt = hip.transform_forward_dt("DNA", text, len(text) + 1024, 0)
    assert not ok and dt == 9, "SMALL_ALPHABET is written before the refusal"
    ok, _, dt = hip.transform_forward_dt("PACK", text, len(text) + 1024, 0)
    assert ok and dt == 9


@pytest.mark.parametrize("idx", range(len(text_cases.BIG_CHAINS)))
def test_four_mib_blocks_bit_exact_and_decode(hip, idx):
    """The block that wraps the index and the one that passes 16,384 entries as a stream of 4 MiB blocks, against the reference's
    stream: hash maps of 2^19 (FPAQ) and 2^17 (NONE) slots. Decoded once (the entropy coders take a 4 MiB block as one chunk)."""
    rec = GOLDEN["big"][idx]
    data = text_cases.big_blocks()
    assert md5(data) == rec["input_md5"]
    _stream(hip, data, rec, len(text_cases.BIG_KINDS), runs=False)


def test_cpp_text_mirror():
    """The stream classes over chains with TEXT in front, behind a device stage and twice (tests/cpp/text_mirror_test.cpp)."""
    import knzlib
    exe = os.path.join(knzlib.ROOT, "tests", "cpp", "text_mirror_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
