"""Pins the oracle against the unmodified reference compiled into oracle/_ref (skipped where that
build is absent). Randomised inputs beyond the committed golden vectors."""
import hashlib

import numpy as np
import pytest

import knzlib
import vectors


def _inputs():
    rng = np.random.default_rng(2024)
    for i in range(6):
        n = int(rng.integers(33, 90000))
        kind = i % 3
        if kind == 0:
            yield rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 1:
            yield bytes((rng.geometric(0.05 + 0.1 * i, n) % 256).astype(np.uint8))
        else:
            a = rng.integers(0, 4, n, dtype=np.uint8)
            a[rng.integers(0, n, n // 50)] = 200
            yield bytes(np.repeat(a, rng.integers(1, 6, n))[:n])


def test_entropy_matches_reference(oracle, ref):
    for d in _inputs():
        for e in ["HUFFMAN", "ANS0", "ANS1", "FPAQ", "NONE"]:
            a, ab = oracle.entropy_encode(e, d)
            b, bb = ref.entropy_encode(e, d)
            assert ab == bb and a == b, e
            r, dec = ref.entropy_decode(e, a, len(d))
            assert r == len(d) and dec == d


def test_transforms_match_reference(oracle, ref):
    for d in _inputs():
        for t in ["BWT", "MTFT", "ZRLT", "SRT", "RLT", "LZ", "LZX", "RANK"]:
            cap = len(d) if t == "ZRLT" else len(d) + 2048
            if t in ("LZ", "LZX"):
                cap = len(d) + len(d) // 64 + 18
            ok1, o1 = oracle.forward(t, d, cap, "ANS0")
            ok2, o2, _ = ref.forward(t, d, cap, "ANS0")
            assert bool(ok1) == (ok2 == 1), t
            if ok1:
                assert o1 == o2, t
                # LZ's inverse wants two readable bytes behind its input (LZCodec.cpp:486-490)
                k, back = ref.inverse(t, o1, max(len(d), len(o1)) + 64, src_cap=len(o1) + 2)
                assert k == 1 and back == d
                k, back = oracle.inverse(t, o1, max(len(d), len(o1)) + 64)
                assert k == 1 and back == d


def test_lz_randomised_against_reference(oracle, ref):
    # LZ / LZX on generated inputs that exercise what the fixed vectors do not: matches longer than MAX_MATCH,
    # repeats at every distance class (1, 2, 3 distance bytes), incompressible stretches (the accelerating stride of
    # the literal loop), tiny blocks around MIN_BLOCK_LENGTH, and rejected blocks
    import numpy as np
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, 6000, dtype=np.uint8).tobytes()
    cases = [b"abcdefghabcdefghabcdefg", b"abcdefghabcdefghabcdefgh", bytes(70000), b"abc" * 30000,
             base * 3 + bytes(70000) + base[:3000] * 9, rng.integers(0, 256, 90000, dtype=np.uint8).tobytes()]
    for i in range(6):
        n = int(rng.integers(24, 120000))
        parts = []
        while sum(map(len, parts)) < n:
            k = int(rng.integers(0, 4))
            if k == 0:
                a = int(rng.integers(0, 5000)); parts.append(base[a:a + int(rng.integers(4, 900))])
            elif k == 1:
                parts.append(rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=np.uint8).tobytes())
            elif k == 2:
                parts.append(bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 400)))
            else:
                parts.append(vectors.make(("text", int(rng.integers(16, 4000)), i)))
        cases.append(b"".join(parts)[:n])
    for d in cases:
        for t in ("LZ", "LZX"):
            cap = ((len(d) + 16) if len(d) <= 1024 else len(d) + len(d) // 64) + 2
            ok1, o1 = oracle.forward(t, d, cap)
            ok2, o2, _ = ref.forward(t, d, cap)
            assert bool(ok1) == (ok2 == 1), (t, len(d))
            if ok1:
                assert o1 == o2, (t, len(d))
                assert oracle.inverse(t, o1, len(d) + 64) == (1, d)
                assert ref.inverse(t, o1, len(d) + 64, src_cap=len(o1) + 2)[:2] == (1, d)
            # destination below getMaxEncodedLength: the codec refuses (LZCodec.cpp:131-132); the harness goes through
            # TransformSequence, which would swap in a larger buffer first, so only the restatement is asked here
            assert oracle.forward(t, d, cap - 1)[0] == 0


def test_sbrt_modes_match_reference(oracle, ref):
    # SBRT(mode) constructed directly: RANK (also reachable as transform id 8) and TIMESTAMP (no id)
    for d in _inputs():
        x = oracle.forward("BWT", d, len(d) + 64)[1] if len(d) else d
        for data in (d, x):
            for name, mode in (("RANK", 2), ("TIMESTAMP", 3)):
                ok1, o1 = oracle.forward(name, data, len(data))
                ok2, o2 = ref.sbrt(mode, True, data)
                assert bool(ok1) == (ok2 == 1) and o1 == o2, name
                assert ref.sbrt(mode, False, o1)[1] == data and oracle.inverse(name, o1, len(data))[1] == data


def test_streams_match_reference(oracle, ref):
    d = vectors.make(("mixed", 700001, 11))
    for t, e, bs, ck in [("BWT+MTFT+ZRLT", "ANS0", 65536, 0), ("BWT+SRT+ZRLT", "FPAQ", 262144, 32),
                         ("RLT+ZRLT", "HUFFMAN", 16384, 64), ("NONE", "ANS1", 1 << 20, 0),
                         ("LZX", "ANS1", 262144, 0), ("LZ+ZRLT", "HUFFMAN", 65536, 32),
                         # more than four stages: the skip flags get a byte of their own in the block header
                         ("BWT+RANK+ZRLT+RLT+MTFT", "ANS0", 65536, 0), ("RLT+BWT+RANK+ZRLT+MTFT+SRT", "HUFFMAN", 262144, 32),
                         ("RLT+BWT+SRT+ZRLT+RLT+MTFT+ZRLT", "FPAQ", 65536, 64)]:
        for jobs in (1, 3):
            # the job count selects buffer slots, hence capacities, hence ZRLT's success on short last blocks
            rc1, a = oracle.compress(d, t, e, bs, ck, jobs=jobs)
            rc2, b = ref.compress(d, t, e, bs, jobs=jobs, checksum=ck)
            assert rc1 == 0 and rc2 == 0 and a == b, (t, e, jobs)
        rc, back = ref.decompress(a, len(d) + 16, jobs=2)
        assert rc == 0 and back == d


def test_checksums_match_reference(oracle, ref):
    # XXHash32/64 are exercised through the -x32 / -x64 stream paths above; check a few raw values too
    d = vectors.make(("text", 1000, 2))
    assert oracle.L.knzo_xxhash32(knz_buf(d), len(d), 0x4B414E5A) != 0
    assert oracle.L.knzo_xxhash64(knz_buf(d), len(d), 0x4B414E5A) != 0


def knz_buf(b):
    import ctypes as C
    return (C.c_uint8 * len(b)).from_buffer_copy(b)


def test_reference_block_range_semantics():
    """Pins what `from` / `to` mean in the reference (io/CompressedInputStream.cpp:836-868): 1-based block ids, blocks with
    from <= id < to are delivered. The host layer's setBlockRange / Context constructor is tested against the same rule in
    tests/cpp/host_mirror_test.cpp (testBlockRange)."""
    import ctypes as C
    so = knzlib.ensure_ref()
    if so is None:
        pytest.skip("reference build not available")
    L = C.CDLL(so)
    u8p = C.POINTER(C.c_uint8)
    L.ref_decompress_range.restype = C.c_int
    L.ref_decompress_range.argtypes = [u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    bs = 16384
    d = vectors.make(("mixed", 7 * bs + 777, 4))
    rc, enc = knzlib.Ref().compress(d, "BWT+MTFT+ZRLT", "HUFFMAN", bs, jobs=1)
    assert rc == 0
    src = (C.c_uint8 * len(enc)).from_buffer_copy(enc)
    for lo_id, hi_id in [(1, 0x7FFFFFFF), (3, 6), (1, 2), (8, 9), (5, 100), (9, 12)]:
        out = (C.c_uint8 * (len(d) + 16))()
        ol = C.c_size_t(0)
        rc = L.ref_decompress_range(src, len(enc), 1, lo_id, hi_id, out, len(d) + 16, C.byref(ol))
        lo, hi = min(len(d), (lo_id - 1) * bs), min(len(d), (hi_id - 1) * bs)
        assert rc == 0 and C.string_at(out, ol.value) == d[lo:hi], (lo_id, hi_id, rc, ol.value, hi - lo)


def test_chains_left_out_of_the_soak_have_no_reference_behaviour(ref):
    """tests/test_gpu_parity.py::test_randomised_soak leaves out BWT+ZRLT and BWT+RLT+ZRLT. This pins why: when the stage behind the
    BWT is skipped or expands, the unmodified reference writes a stream that the unmodified reference refuses (error 13, "Block 1
    incorrectly decompressed") -- and not even the same stream every time (the bytes depend on what its buffers held before) -- so
    there is nothing for a device path to be bit-exact with. If a later reference fixes this, this test fails and the chains go
    back into the soak."""
    for t, e, spec, bs in [("BWT+ZRLT", "NONE", ("rand", 40000, 1), 16384), ("BWT+RLT+ZRLT", "ANS0", ("rand", 40000, 1), 16384),
                           ("BWT+ZRLT", "HUFFMAN", ("mixed", 700001, 11), 65536)]:
        d = vectors.make(spec)
        rc, out = ref.compress(d, t, e, bs, jobs=1)
        assert rc == 0, (t, e)
        rc2, back = ref.decompress(out, len(d))
        assert rc2 != 0 or back != d, (t, e, "the reference now decodes its own stream: put the chain back into the soak")


def test_first_gen_damage_fixture_is_the_case_list_and_the_oracle_agrees(oracle):
    """tests/golden/first_gen_damage.json (written by tests/golden/make_first_gen_damage.py from the reference build) holds exactly the
    cases of tests/first_gen_damage.py, in their order, and the restatement in oracle/ gives every recorded decision, length and md5.
    Needs no reference build: this is what ties the fixture the GPU tests read to the oracle they encode with."""
    import first_gen_damage as fgd
    cases, dropped = fgd.load()
    have = {fgd.key(r) for r in cases} | {fgd.key(r) for r in dropped}
    listed = [fgd.key(r) for r in fgd.enumerate_cases(oracle)]
    assert len(have) == len(cases) + len(dropped) == len(listed) and have == set(listed)
    assert [fgd.key(r) for r in cases] == [k for k in listed if k not in {fgd.key(r) for r in dropped}]
    lz = [r for r in cases if r["stage"] == "LZ" and not r["intact"]]
    accepted = sum(r["ok"] for r in lz)
    assert 4 * accepted >= len(lz) and 4 * (len(lz) - accepted) >= len(lz), (accepted, len(lz))       # the draw tests both sides
    for r in cases:
        ok, out = oracle.inverse(r["transform"], fgd.block(oracle, r), r["cap"])
        assert (1 if ok else 0) == r["ok"], r
        if ok:
            assert len(out) == r["len"] and (r["md5"] is None or hashlib.md5(out).hexdigest() == r["md5"]), r
        if r["intact"] and r["ok"]:
            assert out == fgd.plain(r), r


def test_damaged_first_gen_blocks_match_reference(oracle, ref):
    """The same cases against the reference build itself: the fixture is what the reference answers today, with two bytes behind an LZ
    block (what its decoder asks for, LZCodec.cpp:486-490) and with 4 KiB of zeros."""
    import first_gen_damage as fgd
    cases, dropped = fgd.load()
    n = 0
    for r in cases:
        if r["source"] != "reference":
            assert r["cap"] < r["cut"], r                    # (a destination shorter than the input: the harness cannot be asked)
            continue
        blk = fgd.block(oracle, r)
        for pad in ((2, 4096) if r["stage"] == "LZ" else (0,)):
            ok, out = ref.inverse(r["transform"], blk, r["cap"], src_cap=len(blk) + pad)
            assert (1 if ok == 1 else 0) == r["ok"], (r, pad)
            if ok == 1:
                assert len(out) == r["len"] and (r["md5"] is None or hashlib.md5(out).hexdigest() == r["md5"]), (r, pad)
        n += 1
    assert n >= 700


def test_lzx_extensions_read_behind_the_block(oracle, ref):
    """LZX, text(60000, 3), header byte 8 changed from 136 to 183 (nDist + 47): the length extensions start 47 bytes late, and the
    decoder, which never looks for the end of the block when it reads one (readLength, LZCodec.hpp:212-225; the two guard bytes of
    LZCodec.cpp:486-490 are all it asks for), reads the last of them behind the block. What it finds there decides: with zeros behind
    the block -- what oracle/lz.c and the device's byte windows (LzByteWin) read there -- the reference accepts and returns the 59,983
    bytes the oracle returns; with the two guard bytes alone it reads the heap, and refused when this was written. The case is
    therefore not in the fixture (listed under "dropped" there); the restatement needed no change."""
    import first_gen_damage as fgd
    import lz_decoder_cases
    d = lz_decoder_cases.blocks()["text"]
    ok, enc = oracle.forward("LZX", d, lz_decoder_cases.forward_cap(len(d)))
    assert ok and enc[8] == 136
    blk = bytearray(enc); blk[8] = 183; blk = bytes(blk)
    assert any(r["case"] == "nDist+47" for r in fgd.load()[1])
    for cap in (len(d), len(d) + 64):
        ok1, o1 = oracle.inverse("LZX", blk, cap)
        ok2, o2 = ref.inverse("LZX", blk, cap, src_cap=len(blk) + 4096)
        assert ok1 == 1 and ok2 == 1 and len(o1) == 59983 and o1 == o2


def test_bwt_mode_byte_of_eight_one_byte_indexes(oracle, ref):
    """BWT, text of 300 and of 5,000 bytes (seed 3), mode byte 13 (eight indexes of two bytes) changed to 12 (eight of one byte): the
    header is 8 bytes shorter, the block n + 8 bytes, and every byte read as an index is in range. The reference accepts and returns
    n + 8 bytes -- into a destination that holds them. BWT::inverse refuses a block longer than its destination (BWT.cpp:147-151), and
    so does oracle/transforms.c: asked with a capacity of n the restatement refuses, which is where it seemed to disagree; the
    reference's harness cannot be given less than the input's length (TransformSequence). With equal capacities the two agree on
    decision, length and bytes at every capacity the harness takes."""
    for n in (300, 5000):
        d = vectors.make(("text", n, 3))
        ok, enc = oracle.forward("BWT", d, len(d) + 64)
        assert ok and enc[0] == 13 and len(enc) == n + 17
        blk = bytes([12]) + enc[1:]
        for cap in (len(enc), len(enc) + 64):
            ok1, o1 = oracle.inverse("BWT", blk, cap)
            ok2, o2 = ref.inverse("BWT", blk, cap)
            assert ok1 == 1 and ok2 == 1 and len(o1) == n + 8 and o1 == o2, (n, cap)
        assert oracle.inverse("BWT", blk, n + 8)[0] == 1 and oracle.inverse("BWT", blk, n + 7)[0] == 0 and oracle.inverse("BWT", blk, n)[0] == 0
