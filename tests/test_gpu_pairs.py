"""Every ordered pair of the 14 device transforms through the code the stages share (api.hip, sequence.hip: the buffer stride and the
capacities a stage receives in second position, the skip-flag byte, the data type a stage leaves for the one behind it, the per-lane
scratch of the decode ranges): 196 chains over one input of nine blocks of 16 KiB and a copy block, in front of NONE (pass A) and in
front of a rotation of the eight coders, the checksum widths and three job counts (pass B). Expected lengths and digests are the
reference's, from tests/golden/pairs.json (tools/make_pair_golden.py, pinned by tests/test_pair_golden.py); the input makes every stage
that can refuse a block both take and refuse some. One test per first stage.

The typed table (tests/golden/pairs_typed.json) adds EXE, TEXT and DNA, which read the data type as well as set it: the 93 ordered pairs
of the 17 stages that hold one of them, over fourteen blocks and a copy block (the nine above, x86 and ARM64 code, ACGT, an ELF file,
text). The reference writes and reads back every one of them, so none is left out. One test per first stage again."""
import hashlib
import importlib
import json
import os
import time

import numpy as np
import pytest

import knzlib
import pair_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairs.json")))
GOLDEN_TYPED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairs_typed.json")))
KNZ_ERR_INVALID_CODEC = 3            # include/knz_hip.h
HEADLINE = {"chain": "BWT+MTFT+ZRLT", "entropy": "ANS0", "checksum": 0, "jobs": 1}
_data = {}
_ref = []


def md5(b):
    return hashlib.md5(b).hexdigest()


def data(make=cases.make_input, golden=GOLDEN):
    if make not in _data:
        d = make()
        assert md5(d) == golden["input_md5"] and len(d) == golden["n"]
        _data[make] = d
    return _data[make]


def reference():
    """The reference build, for the streams the device refuses to write. Its absence is a failure, not a skip."""
    if not _ref:
        _ref.append(knzlib.Ref())
    return _ref[0]


def encode(hip, d, rec):
    framing = importlib.import_module("kanzi_amd.framing")
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    p = hip.params(rec["chain"], rec["entropy"], cases.BS, rec["checksum"], jobs=rec["jobs"])
    hdr, hb = framing.make_header(p.entropy_type, p.transform_type, cases.BS, rec["checksum"], len(d))
    cap = hip.encode_bound(p, len(d)) + 64
    if p.entropy_type in hipapi.BINARY_CODERS:
        cap += 32 * len(d)                  # knz_hip_encode_bound is these coders' first tier (include/knz_hip.h)
    d_in, d_out = hip.malloc(len(d) + 64), hip.malloc(cap)
    try:
        hip.h2d(d_in, d)
        bits = hip.encode_blocks(p, d_in, len(d), d_out, cap, prologue=hdr, prologue_bits=hb)
        return hip.d2h(d_out, (bits + 7) // 8), hb
    finally:
        hip.free(d_in)
        hip.free(d_out)


def decode(hip, enc, rec, start_bit, n):
    p = hip.params(rec["chain"], rec["entropy"], cases.BS, rec["checksum"], jobs=rec["jobs"])
    d_in, d_out = hip.malloc(len(enc) + 4096), hip.malloc(n + 2 * cases.BS + 64)
    try:
        hip.h2d(d_in, enc + bytes(64))
        ob, _, _ = hip.decode_blocks(p, d_in, 8 * len(enc), start_bit, d_out, n + cases.BS)
        return hip.d2h(d_out, ob)
    finally:
        hip.free(d_in)
        hip.free(d_out)


def first_differing_block(got, want, start_bit):
    """Where two streams part, by the block length prefixes of both: the first block whose framed bits (prefix and payload) differ."""
    sharded = importlib.import_module("kanzi_amd.sharded")
    frames = []
    for s in (got, want):
        try:
            pos, end = sharded.walk_blocks(s, start_bit)
        except ValueError as ex:
            return "the length prefixes of the %s stream cannot be walked (%s)" % ("device's" if s is got else "reference's", ex)
        pos.append(end)
        v = int.from_bytes(s, "big")
        frames.append([(b - a, (v >> (8 * len(s) - b)) & ((1 << (b - a)) - 1)) for a, b in zip(pos, pos[1:])])
    for k, (g, w) in enumerate(zip(*frames)):
        if g != w:
            return "block %d is the first that differs (%d framed bits, the reference's has %d)" % (k, g[0], w[0])
    return "the first %d blocks agree; the device wrote %d blocks, the reference %d" % (min(map(len, frames)), len(frames[0]), len(frames[1]))


def where(d, rec, enc, hb):
    """For the message of a digest mismatch: the reference's stream is computed and compared block by block."""
    rc, want = reference().compress(d, rec["chain"], rec["entropy"], cases.BS, jobs=rec["jobs"], checksum=rec["checksum"], orig_size=len(d))
    return first_differing_block(enc, want, hb) if rc == 0 else "the reference's call failed (code %d)" % rc


def one_pair(hip, L, d, ps, rec, refused):
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    what = (ps, rec["chain"], rec["entropy"], rec["checksum"], rec["jobs"])
    if refused:
        # the device LZ stages do not read the data type the first stage leaves, so the chain is refused rather than written differently
        # from the reference; the decoder needs no data type (the minimum match is in the block) and must read the reference's stream
        with pytest.raises(hipapi.KnzError) as ex:
            encode(hip, d, rec)
        assert ex.value.code == KNZ_ERR_INVALID_CODEC, what
        rc, enc = reference().compress(d, rec["chain"], rec["entropy"], cases.BS, jobs=rec["jobs"], checksum=rec["checksum"], orig_size=len(d))
        assert rc == 0, what
        hb = rec["header_bits"]
    else:
        enc, hb = encode(hip, d, rec)
        assert hb == rec["header_bits"], what
    if (len(enc), md5(enc)) != (rec["knz_len"], rec["knz_md5"]):
        what += (where(d, rec, enc, hb),)        # in pass A the transforms' bytes are in that block unhidden
    assert (len(enc), md5(enc)) == (rec["knz_len"], rec["knz_md5"]), what
    for parts in (3, 1) if ps == "A" else (3,):
        assert L.knz_hip_tune(b"dec_parts", parts) == 0
        assert decode(hip, enc, rec, hb, len(d)) == d, what + (parts,)


@pytest.mark.parametrize("first", cases.T)
def test_every_second_stage_behind(hip, first):
    """`first` in front of each of the 14 stages, both passes: the device writes the reference's stream (for {PACK, MM, UTF, ROLZX} +
    {LZ, LZX} it refuses to, with the invalid-codec code, and is given the reference's) and reads it back as three block ranges, in
    pass A also as one. Cases the fixture leaves out (the reference cannot read, or does not repeat, its own stream) are not run.
    Afterwards the context still round-trips the headline chain."""
    L = importlib.import_module("kanzi_amd.hipapi").lib()
    d, i = data(), cases.T.index(first)
    try:
        for ps in cases.PASSES:
            recs = cases.records(GOLDEN, ps)
            t0, compared = time.time(), 0
            for j in range(14):
                rec = recs[14 * i + j]
                if "left_out" in rec:
                    continue
                one_pair(hip, L, d, ps, rec, cases.refused_when_encoding(i, j))
                compared += 1
            print("%s+*: pass %s, %d cases, %.2f s" % (first, ps, compared, time.time() - t0))
            assert compared >= 13, (first, ps, compared)
    finally:
        L.knz_hip_tune(b"dec_parts", 3)
    enc, hb = encode(hip, d, HEADLINE)
    assert decode(hip, enc, HEADLINE, hb, len(d)) == d


def runs_of(alphabet, n, seed):
    rng = np.random.default_rng(seed)
    out = bytearray(alphabet)                       # every symbol at least once
    while len(out) < n:
        out += bytes([alphabet[int(rng.integers(0, len(alphabet)))]]) * int(rng.geometric(0.3))
    return bytes(out[:n])


def test_rlt_reads_and_leaves_the_data_type(hip):
    """RLT is no stage of the typed table, but behind one it reads the data type, and in front of one it may leave a type (the typed
    table found it judging typed blocks anew: TEXT+RLT in front of CM). The stage by itself with the escape search on, the reference's
    RLT as the yardstick: a block that comes with a type is not looked at again (ACGT and base64 blocks preset TEXT, MULTIMEDIA, BIN
    or SMALL_ALPHABET are transformed; preset BASE64, DNA or UTF8 every block is refused), and on a block that comes without one
    the type detection finds (DNA, NUMERIC, BASE64, BIN, SMALL_ALPHABET or none) stays on it for the stages behind."""
    b64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
    inputs = {"acgt": runs_of(b"ACGT", 4001, 1), "three": runs_of(b"Af\x8b", 4001, 2), "numeric": runs_of(b"0123456789,. ", 4001, 3),
              "base64": runs_of(b64, 4001, 4), "all256": runs_of(bytes(range(256)), 4001, 5), "words": runs_of(b"etaoin shrdlu\n", 4001, 6)}
    found = set()
    for name, d in inputs.items():
        for preset in (0, 1, 2, 5, 6, 7, 8, 9):
            ok, want, left = reference().forward_dt("RLT", d, len(d) + 64, preset)
            got = hip.transform_forward_dt("RLT", d, len(d) + 64, preset)
            assert got[0] == ok and got[2] == left and (not ok or got[1] == want), (name, preset, ok, left, got[0], got[2])
            if preset == 0:
                found.add((ok, left))
    assert found == {(0, 6), (1, 9), (1, 4), (0, 5), (1, 7), (1, 0)}, found


@pytest.mark.parametrize("first", cases.T_TYPED)
def test_every_typed_pair_behind(hip, first):
    """The typed table: an older `first` in front of EXE, TEXT and DNA (6 cases), a new one in front of each of the 17 stages (34), both
    passes. As above: the device writes the reference's stream (for {EXE, TEXT, DNA} + {LZ, LZX} it refuses to and is given the
    reference's) and reads it back as three block ranges, in pass A also as one. Nothing is left out, so every case must have run."""
    L = importlib.import_module("kanzi_amd.hipapi").lib()
    d, i = data(cases.make_typed_input, GOLDEN_TYPED), cases.T_TYPED.index(first)
    seconds = [j for j in range(17) if i >= 14 or j >= 14]
    try:
        for ps in cases.PASSES:
            recs = cases.records_typed(GOLDEN_TYPED, ps)
            t0, compared = time.time(), 0
            for j in seconds:
                rec = recs[i, j]
                assert "left_out" not in rec, rec
                one_pair(hip, L, d, ps, rec, cases.refused_when_encoding(i, j, cases.T_TYPED, cases.SETS_TYPE_TYPED))
                compared += 1
            print("typed %s+*: pass %s, %d cases, %.2f s" % (first, ps, compared, time.time() - t0))
            assert compared == len(seconds) == (17 if i >= 14 else 3), (first, ps, compared)
    finally:
        L.knz_hip_tune(b"dec_parts", 3)
    enc, hb = encode(hip, d, HEADLINE)
    assert decode(hip, enc, HEADLINE, hb, len(d)) == d
