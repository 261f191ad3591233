"""The inverse BWT (csrc/bwt.hip) on the device, path by path. The encoded blocks are the oracle's; the device must return the input.

  * Single blocks at the sizes where the stage changes its course (tests/bwt_inverse_cases.py: rows of the walk, one and eight primary
    indexes, tiles and segments of the counting sort) with five kinds of content, under the defaults and under each of the stage's knobs:
    bwt_inv_wide (the 8-byte link records, which a batch takes by itself only with a block above 8 MiB), bwt_inv_jump_all (pointer jumping
    over all rows: the escape for blocks the ruler walk refuses) and bwt_inv_ruler_log (one row in 4 and one in 256 a ruler).
  * Blocks of 2^23 and 2^23 + 1 bytes without a knob: the last block of 4-byte records, whose positions take all 23 bits of their field,
    and the first of 8-byte ones.
  * A batch whose blocks reach the stage with eight different lengths (an RLT stage in front), encoded and decoded, under every setting
    and with the stage cut into one part and into four.
  * Blocks with damaged headers (tests/golden/first_gen_damage.json: the reference's decisions): accept / refuse and the length.

A test that sets a knob puts the default back."""
import hashlib
import importlib

import pytest

import bwt_inverse_cases as cases
import first_gen_damage as fgd
import knzlib
from test_gpu_parity import gpu_compress, gpu_decompress

pytestmark = pytest.mark.gpu

# name -> ((knob, value, default), ...)
SETTINGS = {
    "defaults": (),
    "wide": ((b"bwt_inv_wide", 1, 0),),
    "jump_all": ((b"bwt_inv_jump_all", 1, 0),),
    "ruler_log_2": ((b"bwt_inv_ruler_log", 2, 3),),
    "ruler_log_8": ((b"bwt_inv_ruler_log", 8, 3),),
}

_encoded = {}


def lib():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.hipapi").lib()


class knobs:
    def __init__(self, setting):
        self.setting = setting

    def __enter__(self):
        for knob, value, _ in self.setting:
            assert lib().knz_hip_tune(knob, value) == 0

    def __exit__(self, *exc):
        for knob, _, default in self.setting:
            lib().knz_hip_tune(knob, default)


def single_blocks(oracle):
    """[(name, input, the oracle's encoded block)], computed once."""
    if "single" not in _encoded:
        out = []
        for name, d in cases.single_blocks():
            ok, enc = oracle.forward("BWT", d, len(d) + 64)
            assert ok and len(enc) == len(d) + cases.header_len(enc), name
            out.append((name, d, enc))
        _encoded["single"] = out
    return _encoded["single"]


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_single_blocks_at_every_path_boundary(hip, oracle, setting):
    with knobs(SETTINGS[setting]):
        for name, d, enc in single_blocks(oracle):
            ok, back = hip.transform_inverse("BWT", enc, len(d))
            assert ok == 1 and back == d, (setting, name)


def record_width(hip, enc, n):
    """Decodes the block with the timing of kernels on: (ok, bytes, width of the link records the stage reports among its kernel times)."""
    hip.set_profiling(True)
    try:
        ok, back = hip.transform_inverse("BWT", enc, n)
        names = {name for name, ms, launches in hip.kernel_times()}
    finally:
        hip.set_profiling(False)
    width = {4 for w in ("bwt_i_records_4_byte",) if w in names} | {8 for w in ("bwt_i_records_8_byte",) if w in names}
    assert len(width) == 1, names
    return ok, back, width.pop()


def test_narrow_records_end_at_8_mib_exactly(hip, oracle):
    """inv_narrow's `<=` and the 23-bit position of the 4-byte records at their limit: a block of INV_NARROW_MAX bytes is the last one with
    4-byte records, one of a byte more the first with 8-byte ones. No knob is set."""
    text = knzlib.corpus().text(cases.INV_NARROW_MAX + 1, 1)
    for n, width in ((cases.INV_NARROW_MAX, 4), (cases.INV_NARROW_MAX + 1, 8)):
        d = text[:n]
        ok, enc = oracle.forward("BWT", d, n + 64)
        assert ok
        ok, back, w = record_width(hip, enc, n)
        assert ok == 1 and len(back) == n and hashlib.md5(back).digest() == hashlib.md5(d).digest(), n
        assert w == width, n


def test_wide_knob_selects_the_8_byte_records(hip, oracle):
    """The proof that bwt_inv_wide takes: a block of 4,097 bytes has 4-byte records by itself and 8-byte ones under the knob (the stage
    reports the width it used among the kernel times, csrc/bwt.hip: launch_bwt_inverse)."""
    name, d, enc = [x for x in single_blocks(oracle) if x[0] == "text_4097"][0]
    ok, back, w = record_width(hip, enc, len(d))
    assert ok == 1 and back == d and w == 4
    with knobs(SETTINGS["wide"]):
        ok, back, w = record_width(hip, enc, len(d))
        assert ok == 1 and back == d and w == 8
    ok, back, w = record_width(hip, enc, len(d))
    assert ok == 1 and back == d and w == 4


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_ragged_batch_encodes_and_decodes(hip, oracle, setting):
    """Eight blocks that reach the BWT stage with eight lengths between 1 and 16,384 bytes (RLT in front; two blocks RLT refuses): the
    device writes the oracle's stream -- which equals the reference build's, tests/test_oracle_vs_ref.py -- and reads it back, with the
    BWT stages of the batch as one part and as four."""
    assert cases.ragged_stage_lengths(oracle) == cases.RAGGED_STAGE_LENGTHS
    data = b"".join(cases.ragged_data())
    L = lib()
    try:
        with knobs(SETTINGS[setting]):
            for split in (1, 4):
                assert L.knz_hip_tune(b"bwt_split", split) == 0
                for transform, entropy in cases.RAGGED_CHAINS:
                    rc, want = oracle.compress(data, transform, entropy, cases.RAGGED_BS, headerless=1)
                    assert rc == 0
                    out, bits, hb = gpu_compress(hip, data, transform, entropy, cases.RAGGED_BS, headerless=1)
                    assert out == want, (setting, split, transform)
                    assert gpu_decompress(hip, want, transform, entropy, cases.RAGGED_BS, len(data), 0) == data, (setting, split, transform)
    finally:
        L.knz_hip_tune(b"bwt_split", 3)


@pytest.mark.parametrize("setting", ("defaults", "wide"))
def test_header_decisions_are_the_references(hip, oracle, setting):
    """Blocks of 300 and 5,000 bytes of text with every header byte set to 0, 0xFF, b^1, b^4, b^0x80 and b+1 in turn, cut to the header,
    to the header and a byte, without their last byte, and into a destination a byte short: the device accepts and refuses what the
    reference does (tests/golden/first_gen_damage.json) and returns the same length.

    Bytes are compared only where the block is as it was encoded. An accepted block with a wrong but in-range primary index is walked as
    one chain from index 0 by the device (the other seven indexes only have to be in range) and as eight chains by the reference, so
    their bytes cannot agree; the decision and the length do. A refused block never gets beyond k_bwt_i_header. The same blocks went
    through the emulated kernels under AddressSanitizer first (tests/test_emu_kernels.py::test_decoders_survive_damaged_input_emulated)."""
    recs = [r for r in fgd.load()[0] if r["stage"] == "BWT"]
    assert len(recs) == 2 * (17 * 6 + 4)
    accepted = 0
    with knobs(SETTINGS[setting]):
        for r in recs:
            ok, out = hip.transform_inverse("BWT", fgd.block(oracle, r), r["cap"])
            assert ok == r["ok"], r
            if ok:
                accepted += 1
                assert len(out) == r["len"], r
                if r["intact"]:
                    assert out == fgd.plain(r), r
    assert 0 < accepted < len(recs)
