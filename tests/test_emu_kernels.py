"""Kernel logic on the CPU: selected .hip files are compiled as plain C++ against the fiber emulation in tools/hipemu
(threads of a workgroup = cooperative fibers, wave intrinsics = 64-lane rendezvous) and their results are compared with
the oracle. This exercises index arithmetic, LDS protocols and wave-level ranking where no GPU exists; it is test
infrastructure only -- the product path never runs this way (the `-m gpu` tests run the real kernels through the C ABI)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import knzlib

ROOT = knzlib.ROOT
EMU = os.path.join(ROOT, "tests", "emu")


def build(name, tmp_path, extra=()):
    knzlib.ensure_oracle()
    exe = str(tmp_path / name)
    cmd = ["g++", "-O1", "-std=c++17", "-x", "c++", "-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "include"), "-I" + EMU,
           "-Wno-unused-value", "-Wno-attributes", "-Wno-format-extra-args", os.path.join(EMU, name + ".cpp"),
           os.path.join(ROOT, "tools", "hipemu", "hipemu.cpp"), "-x", "none", "-L" + os.path.join(ROOT, "oracle"), "-lknz_oracle",
           "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-o", exe] + list(extra)
    subprocess.check_call(cmd)
    return exe


def write_case(path, blocks):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blocks)))
        for b in blocks:
            f.write(struct.pack("<I", len(b)))
            f.write(b)


def test_device_primitives_emulated(tmp_path):
    """csrc/prims.hpp -- the hand-written prefix scans and the segmented stable LSD radix sort that replaced rocPRIM -- against
    std::stable_sort / plain loops: u32 and u64 keys, with and without values, partial digits, empty / tiny / ragged segments,
    constant and low-entropy digits (the one-digit fast path of the counting kernel), sizes from device memory (0 among them), scans
    in place, rs_sort_keep, and -- in every run below, on both paths -- segments of more than RS_GROUP tiles (the second level of the
    column scan). The same primitives on the GPU: tests/test_gpu_prims.py."""
    exe = build("prims_emu", tmp_path)
    # the passes read their keys once (k_rs_hist_all + k_rs_onesweep: tiles learn their predecessors' counts by look-back; tiles are handed
    # out by a ticket counter, so any workgroup order will do -- HIPEMU_ORDER=2 is a permutation) or twice (k_rs_count + k_rs_scatter, KNZ_RS_ONESWEEP=0)
    for args, env in (([], {}), (["quick"], {"HIPEMU_ORDER": "2"}), (["quick"], {"KNZ_RS_ONESWEEP": "0", "HIPEMU_ORDER": "2"})):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
        assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_bwt_forward_kernels_emulated(tmp_path):
    exe = build("bwt_fwd_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(1)
    ramp = bytes((np.arange(20000) % 64).astype(np.uint8))          # period 64: groups of ~312 -> the medium (LDS radix) path
    z = bytearray(24000)                                             # long zero runs: a group above 16384 -> the large path
    for p in rng.integers(0, 24000, 40):
        z[p] = int(rng.integers(1, 256))
    words = [bytes(rng.integers(97, 101, int(rng.integers(2, 6)), dtype=np.uint8)) for _ in range(40)]
    babble = b" ".join(words[int(i)] for i in rng.integers(0, 40, 40000))[:150000]   # many groups that straddle window borders
    # "abcdefg" + 2 random bytes, 3000 times: a group of 3000 whose members all look at different groups (plain LDS radix sort);
    # period-4 and period-700 stretches: groups of ~5000 / ~1000 in which one key holds the majority (split + sort of the rest)
    marked = b"".join(b"abcdefg" + rng.integers(0, 256, 2, dtype=np.uint8).tobytes() for _ in range(3000))
    per4 = bytes((np.arange(20000) % 4).astype(np.uint8)) + c.text(3000, 5)
    unit = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    per700 = unit * 12 + c.text(2000, 6) + unit * 9
    cases = [
        [babble],
        [marked, per4, per700],
        [b"mississippi", b"abcabcabcabcabcabcab", bytes(5), b"a", b"ab", b"zero tail ab\0\0\0" + bytes(9), b"\0\0ab\0\0ab\0\0", c.text(3000, 1), bytes((np.arange(1000) & 255).astype(np.uint8))],
        [c.text(30000, 2), bytes(3000) + c.text(500, 3), ramp, rng.integers(0, 4, 20000, dtype=np.uint8).tobytes()],
        [bytes(z), c.mixed(300000, 2)[250000:290000]],
        [bytes(5000)],                       # a lone block whose round-0 key (position packed in) takes all 64 bits
        [c.text(8000, 7)],
    ]
    for i, blocks in enumerate(cases):
        path = str(tmp_path / ("case%d.bin" % i))
        write_case(path, blocks)
        for order in (("0", "1", "2") if i in (2, 5, 6) else ("0", "2")):       # workgroup dispatch order is not defined: forward, reverse, shuffled
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=dict(os.environ, HIPEMU_ORDER=order))
            assert r.returncode == 0, (i, order, r.stdout[-2000:] + r.stderr[-2000:])
        # the same without the run-length round (run groups refined by doubling like any other group), and with the run groups
        # handed back to the ordinary lists (the path taken when a batch has more run groups than the sort key has index bits)
        if i in (0, 6):                      # (the switches below on the cases with runs, periods and tiny blocks; the two text cases keep the default path)
            continue
        # (round 6: KNZ_BWT_PLAIN_LABELS = 32-bit labels with separate key kernels, the path of blocks above 256 MiB)
        for var in ("KNZ_BWT_NO_RUN_ROUND", "KNZ_BWT_RUN_FALLBACK", "KNZ_BWT_PLAIN_LABELS"):
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=dict(os.environ, **{var: "1"}))
            assert r.returncode == 0, (i, var, r.stdout[-2000:] + r.stderr[-2000:])


def test_bwt_forward_long_common_prefixes_emulated(tmp_path):
    """The shapes of tests/vectors.HARD_CASES at emulator size: copies with edits, X || X, periods 3 / 5 / 7 (large groups all the way),
    period 700 and 520 in medium groups (k_bwt_f_probe: one doubling round instead of ~16), ramps of period 256 and 64 (chain round),
    the Fibonacci word, DNA with repeats, sparse values in zero runs and runs of random lengths (groups the run round leaves tied look
    behind their run), fixed-length records and an image plane."""
    exe = build("bwt_fwd_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(5)
    unit = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    z = bytearray(120000)
    for p in rng.integers(0, len(z), len(z) // 64):
        z[p] = int(rng.integers(1, 4))
    runs = bytearray()
    while len(runs) < 100000:
        runs += bytes([int(rng.integers(0, 3))]) * int(rng.geometric(0.03))
    ramp = lambda n, k, o=0: bytes(((np.arange(n) + o) % k).astype(np.uint8))
    cases = [
        [c.repeats(100000, 3), c.tile(60000, 1, 30000)],
        [c.periodic(30000, 5, 3), c.periodic(29997, 6, 5), c.periodic(30000, 7, 7)],
        [unit * 150 + c.text(2000, 6) + unit * 130, c.periodic(140000, 9, 520)],
        [ramp(80000, 256) + c.text(3000, 1) + ramp(70000, 256, 7), ramp(30000, 64) + c.text(500, 2) + ramp(20000, 64, 3)],
        [c.fibword(60000), c.dna(100000, 4)],
        [bytes(z), bytes(runs[:100000])],
        [c.records(60000, 11, 24, 20), c.records(60000, 12, 100, 93), c.gradient(80000, 13, 1000)],      # a table, an image plane
    ]
    for i, blocks in enumerate(cases):
        path = str(tmp_path / ("hard%d.bin" % i))
        write_case(path, blocks)
        for order in (("0", "2") if i == 2 else ("2",)):
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=1800, env=dict(os.environ, HIPEMU_ORDER=order, KNZ_BWT_STATS="1"))
            assert r.returncode == 0, (i, order, r.stdout[-2000:] + r.stderr[-2000:])
            if i == 2:
                assert r.stderr.count("round h=") <= 2, r.stderr[-1500:]          # the probe took the periodic groups
        if i in (0, 4):                      # copies / Fibonacci word and DNA once more with 32-bit labels and separate key kernels
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=1800, env=dict(os.environ, HIPEMU_ORDER="2", KNZ_BWT_PLAIN_LABELS="1"))
            assert r.returncode == 0, (i, "plain labels", r.stdout[-2000:] + r.stderr[-2000:])
    # the link step for small groups inside long repeats (round 5): text with copied spans, X || X and a block that holds a text three times
    # with edits, with the step tried from the first doubling round on (KNZ_BWT_LINK=4) and with it off -- the same suffix array either way,
    # and X || X in far fewer rounds with it
    t = c.text(40000, 9)
    ed = bytearray(t); ed[777] = 1; ed[22222] = 2
    for name, blocks in (("link_mixed", [c.repeats(100000, 3), c.tile(60000, 1, 30000), t + bytes(ed) + t[:30000], c.dna(100000, 4)]),
                         ("link_xx", [c.tile(60000, 1, 30000), t + bytes(ed) + t[:30000]])):
        path = str(tmp_path / (name + ".bin"))
        write_case(path, blocks)
        rounds, said = {}, {}
        for link in ("4", "0", "1"):
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=1800, env=dict(os.environ, HIPEMU_ORDER="2", KNZ_BWT_STATS="1", KNZ_BWT_LINK=link))
            assert r.returncode == 0, (name, link, r.stdout[-2000:] + r.stderr[-2000:])
            rounds[link] = r.stderr.count("round h=")
            said[link] = "link step:" in r.stderr
        assert said["4"] and not said["0"], (name, said)
        if name == "link_xx":
            assert rounds["4"] < rounds["0"], rounds
    # found by tools/emu_fuzz_bwt.py (seed 7201, case 272) while the step was built: the trial's bit map covers the first block only, and a
    # window of the second block that rode along flagged and looked up positions outside it -- wrong offsets, a wrong suffix array for block 1
    import lzma
    path = str(tmp_path / "link_trial.bin")
    with open(path, "wb") as f:
        f.write(lzma.decompress(open(os.path.join(os.path.dirname(__file__), "golden", "emu_bwt_link_trial_case.bin.xz"), "rb").read()))
    for order in ("0", "2"):
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=1800, env=dict(os.environ, HIPEMU_ORDER=order, KNZ_BWT_LINK="4"))
        assert r.returncode == 0, (order, r.stdout[-2000:] + r.stderr[-2000:])


def test_fpaq_kernels_emulated(tmp_path):
    # encoder phase 1 (probability chains per context family), phase 2 (interval recurrence) and the decoder against oracle/fpaq.c
    exe = build("fpaq_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(3)
    blocks = [c.text(5000, 1), bytes(3000), rng.integers(0, 256, 4000, dtype=np.uint8).tobytes(), b"a", b"ab" * 40,
              c.mixed(300000, 2)[250000:258000], bytes([255]) * 700 + bytes(range(256)) * 3]
    path = str(tmp_path / "fpaq.bin")
    write_case(path, blocks)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # sub-chunk borders (the coder state carries over, the context class restarts): kernels and a private copy of the oracle's
    # sources built with 4 KiB sub-chunks instead of 4 MiB
    objs = []
    for src in sorted(os.listdir(os.path.join(ROOT, "oracle"))):
        if src.endswith(".c"):
            obj = str(tmp_path / (src[:-2] + ".o"))
            subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-DFPAQ_CHUNK=4096u", "-c", os.path.join(ROOT, "oracle", src), "-o", obj])
            objs.append(obj)
    exe2 = str(tmp_path / "fpaq_emu_small")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-x", "c++", "-DKNZ_EMU_FPAQ_CHUNK=4096u", "-I" + os.path.join(ROOT, "tools", "hipemu"),
                           "-I" + os.path.join(ROOT, "include"), "-Wno-unused-value", "-Wno-attributes", "-Wno-format-extra-args",
                           os.path.join(EMU, "fpaq_emu.cpp"), os.path.join(ROOT, "tools", "hipemu", "hipemu.cpp"), "-x", "none"] + objs + ["-o", exe2])
    path2 = str(tmp_path / "fpaq2.bin")
    write_case(path2, [c.text(20000, 1), c.mixed(300000, 2)[250000:262000], bytes(9000)])
    r = subprocess.run([exe2, path2], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_bwt_inverse_kernels_emulated(tmp_path):
    # tile histograms + ballot ranks -> links, splitter walks, dword-gathered stores, against the oracle's forward transform
    exe = build("bwt_inv_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(2)
    cases = [
        [b"ab", b"mississippi", bytes(255), bytes(range(256)), bytes(257), c.text(5000, 1), b"abcabcabcabcabcabcab"],
        [c.text(30000, 2), c.mixed(300000, 2)[250000:262345], rng.integers(0, 4, 9000, dtype=np.uint8).tobytes(), bytes(3000) + c.text(500, 3)],
    ]
    for i, blocks in enumerate(cases):
        path = str(tmp_path / ("inv%d.bin" % i))
        write_case(path, blocks)
        for order in ("0", "2"):
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=dict(os.environ, HIPEMU_ORDER=order))
            assert r.returncode == 0, (i, order, r.stdout[-2000:] + r.stderr[-2000:])
        # the block header of bitstream versions below 6 (BWTBlockCodec.cpp:140-164), written by the oracle, read by k_bwt_i_header<true>
        r = subprocess.run([exe, path, "5"], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (i, "v5", r.stdout[-2000:] + r.stderr[-2000:])


def test_mtft_kernels_emulated(tmp_path):
    # forward and inverse MTFT (4 KiB tiles, two-level scans over the tile tables) against oracle/transforms.c; sizes around tile and
    # segment borders: 1 tile, 2..5 tiles (segments of 2-4 tiles), 70 tiles (segments of 16), ragged tails, empty-ish blocks
    exe = build("mtft_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(5)
    blocks = [c.text(300000, 1)[:287000], bytes(9000), rng.integers(0, 256, 4096, dtype=np.uint8).tobytes(), rng.integers(0, 256, 4097, dtype=np.uint8).tobytes(),
              c.mixed(300000, 2)[250000:270481], b"a", b"abracadabra", bytes(range(256)) * 33, rng.integers(0, 3, 12289, dtype=np.uint8).tobytes(),
              c.text(20000, 9)[:16384]]
    # round 5: shapes for the data-parallel forward kernel (k_mtf_f_rank_par: ranks from counts over the 64 bytes of a chunk) -- every symbol
    # once per chunk, one symbol per chunk, two symbols alternating, 64 distinct symbols cycling with period 65 (a chunk border inside every
    # period), all 256 symbols in descending order, a block that ends inside a chunk
    blocks += [bytes(range(64)) * 200, b"z" * 5000, b"xy" * 3000, bytes(list(range(65)) * 130), bytes(range(255, -1, -1)) * 20,
               rng.integers(0, 256, 64 * 7 + 13, dtype=np.uint8).tobytes(), rng.integers(0, 8, 4096 * 2 + 63, dtype=np.uint8).tobytes()]
    # round 6: the forward kernel ranks run heads only (packs them to the front of the tile, spreads the ranks out again): what a BWT leaves
    # behind (long runs, few heads), tiles just under and over the one-in-eight threshold, runs that cross chunk and tile borders
    o = knzlib.Oracle()
    bw = o.forward("BWT", c.text(70000, 3))[1]
    assert len(bw) >= 70000
    blocks += [bytes(bw), b"".join(bytes([rng.integers(0, 256)]) * int(rng.integers(1, 40)) for _ in range(2000)),
               b"".join(bytes([i & 255]) * 8 for i in range(1024)), b"".join(bytes([i & 255]) * 9 for i in range(1024)),
               b"q" * 63 + b"r" * 65 + b"q" * 4096 + b"s" * 4095 + b"t", bytes(4096) + b"\x01" + bytes(4095)]
    path = str(tmp_path / "mtft.bin")
    write_case(path, blocks)
    for order in ("0", "2"):
        for chain in ("0", "1"):          # KNZ_MTF_CHAIN=1: the byte-serial forward kernel of rounds 2-4
            r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=dict(os.environ, HIPEMU_ORDER=order, KNZ_MTF_CHAIN=chain))
            assert r.returncode == 0, (order, chain, r.stdout[-2000:] + r.stderr[-2000:])
    # 1 KiB tiles (what small batches get)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=dict(os.environ, KNZ_MTF_TILE="1024"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_huffman_decoder_kernels_emulated(tmp_path):
    # header scan (alphabet masks, table-driven Exp-Golomb length deltas, fragment sizes) and chunk decode against the oracle's
    # streams: full and tiny alphabets, single-symbol and raw chunks, several chunks per block, blocks at odd bit offsets
    exe = build("huff_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(8)
    blocks = [c.text(50000, 1), rng.integers(0, 256, 40000, dtype=np.uint8).tobytes(), bytes(20000), b"ab" * 9000, c.mixed(300000, 2)[250000:299000],
              rng.integers(0, 3, 16385, dtype=np.uint8).tobytes(), b"x" * 31, c.text(16384, 3), bytes(range(256)) * 70,
              (rng.integers(0, 256, 30000, dtype=np.uint8) & 0x55).tobytes()]
    # geometric frequencies: codes of 11 and 12 bits and the length limiter (the decoder keeps those in a table of their own), with 40, 120
    # and 256 symbols; and two symbols that are all but absent beside one that fills the chunk
    for nsym, seed in ((40, 21), (120, 22), (256, 23)):
        g = np.random.default_rng(seed).geometric(0.35, 40000)
        blocks.append((np.minimum(g - 1, nsym - 1).astype(np.uint8) * (255 // (nsym - 1)) if nsym < 256 else np.minimum((g - 1) * 7 % 256, 255).astype(np.uint8)).tobytes())
    blocks.append(bytes(16000) + b"\x01\x02" + bytes(16766))
    path = str(tmp_path / "huff.bin")
    write_case(path, blocks)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # the chunk layout of bitstream versions below 6 (HuffmanDecoder.cpp:349-459: one code stream per chunk), k_huff_scan<true> /
    # k_huff_decode<true>
    r = subprocess.run([exe, path, "5"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_ans0_decoder_kernels_emulated(tmp_path):
    # rANS order-0 header scan and chunk decode (four interleaved states, LDS payload ring) against the oracle's streams
    exe = build("ans0_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(9)
    blocks = [c.text(50000, 1), rng.integers(0, 256, 40000, dtype=np.uint8).tobytes(), bytes(20000), b"ab" * 9000, c.mixed(300000, 2)[250000:299000],
              rng.integers(0, 3, 16385, dtype=np.uint8).tobytes(), b"x" * 31, c.text(16384, 3), bytes(range(256)) * 70, b"q" * 33, c.text(70001, 4)]
    # more than 64 chunks in one block (the scan writes its chunk records out 64 at a time), and one exactly at the border
    blocks += [c.text(16384 * 66 + 5, 6), c.text(16384 * 64, 7)]
    path = str(tmp_path / "ans0.bin")
    write_case(path, blocks)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_ans1_decoder_kernels_emulated(tmp_path):
    # rANS order-1: header scan over the 256 contexts of a chunk, per-context slot tables, chunk decode (the context of a symbol is the
    # previous byte of its own quarter) against the oracle's streams: text, noise, few symbols, a single symbol, tiny blocks
    exe = build("ans1_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(19)
    blocks = [c.text(30000, 1), rng.integers(0, 256, 20000, dtype=np.uint8).tobytes(), bytes(9000), b"ab" * 5000, c.mixed(300000, 2)[250000:270000],
              rng.integers(0, 3, 7001, dtype=np.uint8).tobytes(), b"x" * 31, b"q" * 33, c.text(4099, 3)]
    blocks += [c.text(n, 5) for n in (34, 37, 255, 256, 259, 260, 263, 511, 516)]        # quarters around one and two stretches of 64 steps
    path = str(tmp_path / "ans1.bin")
    write_case(path, blocks)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_ans1_encoder_and_bit_assembly_emulated(tmp_path):
    # k_ans1_hist / k_ans1_ctx / k_ans1_encode and the bit assembly with 257 slots per chunk, bit for bit against the oracle
    exe = build("ans1_enc_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(23)
    blocks = [c.text(30000, 1), rng.integers(0, 256, 12000, dtype=np.uint8).tobytes(), bytes(9000), b"ab" * 5000, c.mixed(300000, 2)[250000:265000],
              rng.integers(0, 3, 7001, dtype=np.uint8).tobytes(), b"x" * 31, b"q" * 33, c.text(4099, 3)]
    blocks += [c.text(n, 5) for n in (34, 37, 255, 256, 259, 260, 263, 511, 516)]        # quarters around one and two stretches of 64 steps
    path = str(tmp_path / "ans1e.bin")
    write_case(path, blocks)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_zrlt_kernels_emulated(tmp_path):
    # ZRLT forward (incl. blocks it refuses at capacity n) and inverse against oracle/transforms.c: sparse data, text, zeros, noise,
    # 0xFF / 0xFE escapes, runs across tile borders
    exe = build("zrlt_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(4)
    sp = bytearray(30000)
    for p in rng.integers(0, 30000, 600):
        sp[p] = int(rng.integers(1, 256))
    blocks = [bytes(sp), c.text(20000, 1), bytes(5000), rng.integers(0, 256, 9000, dtype=np.uint8).tobytes(), bytes([0xFF, 0xFE, 0, 0, 0xFF]) * 3000,
              b"\0", b"a", bytes(4096) + b"x" + bytes(4095), c.mixed(300000, 2)[250000:270000], bytes(70000)]
    path = str(tmp_path / "zrlt.bin")
    write_case(path, blocks)
    for order in ("0", "2"):
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900, env=dict(os.environ, HIPEMU_ORDER=order))
        assert r.returncode == 0, (order, r.stdout[-2000:] + r.stderr[-2000:])


def test_ans0_encoder_and_bit_assembly_emulated(tmp_path):
    # k_ans0_stats / k_ans0_encode and the bit assembly kernels, block by block in the per-stage form, bit for bit against the oracle
    exe = build("ans0_enc_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(10)
    t = c.text(40000, 1)
    blocks = [t[:16384], t[16384:20000], t[:16383], t, rng.integers(0, 256, 33000, dtype=np.uint8).tobytes(), bytes(20000), b"ab" * 9000,
              c.mixed(300000, 2)[250000:283000], rng.integers(0, 3, 16385, dtype=np.uint8).tobytes(), b"x" * 31, b"q" * 33, bytes(range(256)) * 70]
    path = str(tmp_path / "ans0e.bin")
    write_case(path, blocks)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("name", ["srt", "rlt", "rank", "timestamp", "lz", "lzx"])
def test_block_serial_transforms_emulated(tmp_path, name):
    """SRT, RLT, RANK / TIMESTAMP (SBRT) and LZ / LZX: the wave-per-block kernels against the oracle, forward (same accept / refuse
    decision and bytes at the same capacity) and inverse. Where a kernel counts on a wave executing its memory operations in
    program order across lanes, KNZ_WAVE_ORDER() marks the spot for the emulation (csrc/common.hpp)."""
    exe = build(name + "_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(12)
    runs = bytearray()
    while len(runs) < 30000:
        runs += bytes([int(rng.integers(0, 256))]) * int(rng.geometric(0.05))
    blocks = [c.text(20000, 1), bytes(5000), rng.integers(0, 256, 9000, dtype=np.uint8).tobytes(), bytes(runs[:30000]), b"\0", b"a", b"abcabcabcabcabcabcabcabc" * 50,
              c.mixed(300000, 2)[250000:270000], bytes(40000), c.text(30000, 5), rng.integers(0, 4, 12000, dtype=np.uint8).tobytes(), b"xy" * 17]
    path = str(tmp_path / "xf.bin")
    write_case(path, blocks)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    if name == "srt":
        # the inverse's three waves talk through LDS rings: the same with the emulator visiting the waves of a workgroup last to first
        path2 = str(tmp_path / "xf2.bin")
        write_case(path2, [blocks[0], blocks[3][:9000], blocks[10], blocks[11]])
        r = subprocess.run([exe, path2], capture_output=True, text=True, timeout=1500, env=dict(os.environ, HIPEMU_WAVE_ORDER="1"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    if name in ("lz", "lzx"):
        # the token layout of bitstream versions below 6 (LZCodec.cpp:614-760), written by the oracle, read by k_lz_inverse<true>
        r = subprocess.run([exe, path, "5"], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        # the decoder is two: the data-parallel one (k_lz_i_parse, k_lz_i_expand, k_lz_i_jump, k_lz_i_emit; the default, above) and the
        # one-wave-per-block k_lz_inverse it falls back to
        for ver in ([], ["5"]):
            r = subprocess.run([exe, path] + ver, capture_output=True, text=True, timeout=1500, env=dict(os.environ, KNZ_LZ_SERIAL_DECODE="1"))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    if name == "lzx":
        # a block whose sections span several tiles of the parallel parse (more than 4096 tokens, more than 8192 bytes of length
        # extensions); no block may need the serial parse (the harness says so under KNZ_EMU_VERBOSE)
        path3 = str(tmp_path / "xf3.bin")
        write_case(path3, [c.text(440000, 3)])
        r = subprocess.run([exe, path3], capture_output=True, text=True, timeout=1500, env=dict(os.environ, KNZ_EMU_VERBOSE="1"))
        assert r.returncode == 0 and "k_lz_i_parse" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_huffman_encoder_and_bit_assembly_emulated(tmp_path):
    # k_huff_encode (code lengths, canonical codes, header, fragments) and the bit assembly, bit for bit against the oracle
    exe = build("huff_enc_emu", tmp_path)
    c = knzlib.corpus()
    rng = np.random.default_rng(13)
    t = c.text(40000, 2)
    blocks = [t[:16384], t[16384:20000], t, rng.integers(0, 256, 33000, dtype=np.uint8).tobytes(), bytes(20000), b"ab" * 9000,
              c.mixed(300000, 2)[250000:283000], rng.integers(0, 3, 16385, dtype=np.uint8).tobytes(), b"x" * 31, b"q" * 33, bytes(range(256)) * 70,
              (rng.integers(0, 256, 30000, dtype=np.uint8) & 0x0F).tobytes()]
    # geometric frequencies: long codes, the length limiter, canonical codes over many lengths
    for nsym, seed in ((40, 31), (120, 32), (256, 33)):
        g = np.random.default_rng(seed).geometric(0.35, 40000)
        blocks.append((np.minimum(g - 1, nsym - 1).astype(np.uint8) * (255 // (nsym - 1)) if nsym < 256 else np.minimum((g - 1) * 7 % 256, 255).astype(np.uint8)).tobytes())
    path = str(tmp_path / "huffe.bin")
    write_case(path, blocks)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_decoders_survive_damaged_input_emulated(tmp_path):
    """src/test/TestMalformedStream.cpp in spirit, below the C ABI and on the CPU: the decoder and inverse kernels on damaged input
    (bit flips, overwritten bytes and ranges, zeroed tails; tests/emu/emu_corrupt.hpp) must neither touch memory outside their
    buffers (the drivers are built with AddressSanitizer here: LDS arrays are globals, device buffers heap blocks), nor deadlock
    (the emulator's scheduler aborts), nor run away (timeouts). What they decode is not compared."""
    c = knzlib.corpus()
    rng = np.random.default_rng(31)
    blocks = [c.text(20000, 1), rng.integers(0, 256, 9000, dtype=np.uint8).tobytes(), b"ab" * 4000, c.mixed(300000, 2)[250000:268000],
              rng.integers(0, 3, 6000, dtype=np.uint8).tobytes(), b"x" * 31, c.text(4099, 3), bytes(3000)]
    path = str(tmp_path / "dmg.bin")
    write_case(path, blocks)
    runs = [("huff_emu", ["6", "5"]), ("ans0_emu", ["6"]), ("ans1_emu", ["6"]), ("fpaq_emu", ["6"]), ("bwt_inv_emu", ["6", "5"]),
            ("lz_emu", ["6", "5"]), ("srt_emu", ["6"]), ("zrlt_emu", ["6"]), ("rlt_emu", ["6"])]       # (tools/emu_damage_fuzz.py: all of them, longer)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=6) as pool:                # (compiles and runs are subprocesses: threads are enough)
        exes = dict(zip([n for n, _ in runs], pool.map(lambda n: build(n, tmp_path, extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"]),
                                                       [n for n, _ in runs])))

        def one(job):
            name, ver, seed = job
            env = dict(os.environ, EMU_CORRUPT=str(seed), ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
            r = subprocess.run([exes[name], path] + ([ver] if ver != "6" else []), capture_output=True, text=True, timeout=900, env=env)
            return job, r
        jobs = [(name, ver, seed) for name, versions in runs for ver in versions for seed in range(1, 5)]
        for job, r in pool.map(one, jobs):
            assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, (job, r.stdout[-500:] + r.stderr[-3000:])
    # the BWT blocks with damaged headers of tests/golden/first_gen_damage.json, taken as they are (the driver's "raw" mode), into
    # destinations of exactly the capacity: what k_bwt_i_header decides is the fixture's decision (the reference's) and length
    import first_gen_damage as fgd
    recs = [r for r in fgd.load()[0] if r["stage"] == "BWT"]
    raw = str(tmp_path / "bwt_raw.bin")
    write_raw_case(raw, recs)
    r = subprocess.run([exes["bwt_inv_emu"], raw, "6", "raw"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0"))
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, r.stdout[-500:] + r.stderr[-3000:]
    check_raw_answers(r.stdout, recs)


def write_raw_case(path, recs):
    """Records of the damage fixture as a case file of blocks taken as they are: u32 count, then per block u32 len, u32 capacity, bytes."""
    import first_gen_damage as fgd
    oracle = knzlib.Oracle()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)))
        for rec in recs:
            b = fgd.block(oracle, rec)
            f.write(struct.pack("<II", len(b), rec["cap"]))
            f.write(b)


def check_raw_answers(stdout, recs):
    lines = [ln.split() for ln in stdout.splitlines() if ln.startswith("block ")]
    assert len(lines) == len(recs)
    for ln, rec in zip(lines, recs):
        ok, length = int(ln[3]), int(ln[5])
        assert ok == rec["ok"] and (not ok or length == rec["len"]), (rec, ok, length)


def test_lz_decoders_on_damaged_fixture_blocks_emulated(tmp_path):
    """The damaged LZ / LZX blocks of tests/golden/first_gen_damage.json through the data-parallel decoder (k_lz_i_pparse, k_lz_i_parse for
    what it hands on) and the one-wave-per-block decoder (k_lz_inverse), built with AddressSanitizer: both give the oracle's decision,
    length and bytes (tests/emu/lz_raw_emu.cpp compares), which are the fixture's. The same blocks on the device:
    tests/test_gpu_lz_decoders.py."""
    import first_gen_damage as fgd
    exe = build("lz_raw_emu", tmp_path, extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"])
    groups = {}
    for rec in fgd.load()[0]:
        if rec["stage"] == "LZ":
            groups.setdefault((rec["transform"], rec["input"][1]), []).append(rec)

    def one(item):
        (transform, name), recs = item
        path = str(tmp_path / ("lz_%s_%s.bin" % (transform, name)))
        write_raw_case(path, recs)
        return item, subprocess.run([exe, path, str(knzlib.TTYPE[transform])], capture_output=True, text=True, timeout=900,
                                    env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0"))
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=6) as pool:
        for (key, recs), r in pool.map(one, sorted(groups.items())):
            assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, (key, r.stdout[-1500:] + r.stderr[-3000:])
            check_raw_answers(r.stdout, recs)
