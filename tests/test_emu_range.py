"""RANGE kernels on the CPU: kanzi-cpp_amd/csrc/range.hip compiled as plain C++ against the fiber emulation in tools/hipemu, compared
with tests/range_model.py (which tests/test_range_model.py pins to the reference's streams). Test infrastructure only: the product
runs the real kernels (tests/test_gpu_range.py)."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np

import range_cases
import range_model
from test_emu_kernels import build

EMU_CASES = [
    ["geom", 1, 100, 30], ["geom", 2, 101, 30], ["geom", 255, 102, 30], ["geom", 1024, 105, 30], ["geom", 4097, 108, 30],
    ["alpha", 1024, 441, 63], ["alpha", 1024, 448, 64], ["alpha", 4097, 455, 65], ["const", 40000, 65], ["ramp", 256], ["ramp", 4096],
    ["pow", 40000, 17, 5, 256], ["rand", 32769, 9], ["mid", 21, 5000], range_cases.UNDERFLOW,
]


def run_cases(exe, tmp_path, cases, order="0"):
    """cases: (mode, count, start bit, in bits, bytes); returns (error, bits, bytes) per case."""
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for mode, count, start, bits, d in cases:
            f.write(struct.pack("<IIIII", mode, count, start, bits, len(d)))
            f.write(d)
    r = subprocess.run([exe, case, res], capture_output=True, text=True, timeout=1800, env=dict(os.environ, HIPEMU_ORDER=order))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = open(res, "rb").read()
    o, out = 0, []
    for _ in cases:
        err, bits, n = struct.unpack_from("<III", d, o)
        o += 12
        out.append((err, bits, d[o:o + n]))
        o += n
    return out


def test_range_encode_and_decode_emulated(tmp_path):
    """Every log range, groups of 6 and 8, one symbol, n == scale, the error spread in rounds, a chunk border, a chunk without payload
    between two coded ones, the underflow branch: the kernels' bits are the model's, and the decoder kernel gives the input back from
    bit 0 and from bit 5."""
    exe = build("range_emu", tmp_path)
    blocks = [range_cases.make(r) for r in EMU_CASES]
    want = [range_model.encode(b) for b in blocks]
    got = run_cases(exe, tmp_path, [(1, 0, 0, 0, b) for b in blocks], "2")
    for r, (enc, bits), (err, gbits, genc) in zip(EMU_CASES, want, got):
        assert gbits == bits and genc == enc, r
    dec = []
    for b, (enc, bits) in zip(blocks, want):
        dec.append((0, len(b), 0, bits, enc))
        shifted = (((0x1F << (8 * len(enc))) | int.from_bytes(enc, "big")) << 3).to_bytes(len(enc) + 1, "big")
        dec.append((0, len(b), 5, 5 + bits, shifted))
    back = run_cases(exe, tmp_path, dec)
    for i, (err, used, out) in enumerate(back):
        b, (enc, bits) = blocks[i // 2], want[i // 2]
        assert err == 0 and out == b and used == bits, (EMU_CASES[i // 2], i & 1)


def test_range_decode_of_damaged_input_emulated(tmp_path):
    """Streams cut at every kind of place, with flipped bits, with a corrupted frequency width and with a frequency sum at the scale,
    under AddressSanitizer (host build of the kernels) with the stream and the output in buffers of their exact sizes: the model's
    verdict where the model refuses, a refusal or some output otherwise, never an access out of bounds."""
    exe = build("range_emu", tmp_path, extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"])
    rng = np.random.default_rng(5)
    cases, want = [], []
    for r in (["geom", 4097, 108, 30], ["alpha", 1024, 448, 64], ["mid", 21, 700], ["ramp", 256]):
        b = range_cases.make(r)
        enc, bits = range_model.encode(b)
        cuts = [0, 1, 2, 7, 9, 40, 100, bits // 2, bits - 61, bits - 60, bits - 28, bits - 1]
        for cut in cuts:
            cases.append((0, len(b), 0, cut, enc[:(cut + 7) // 8]))
            want.append("refused")
        for _ in range(12):
            d = bytearray(enc)
            at = int(rng.integers(0, bits))
            d[at >> 3] ^= 0x80 >> (at & 7)
            cases.append((0, len(b), 0, bits, bytes(d)))
            try:
                out, _ = range_model.decode(bytes(d), len(b), 0, bits)
                want.append(out if len(out) == len(b) else "short")
            except range_model.BadStream:
                want.append("refused")
            except ValueError:
                want.append("refused")
    # a width of 13 at lr 12, and frequencies that sum to the scale: partial alphabet {0, 1, 2}, lr 12
    for freqs, width in (([100, 200], 13), ([2048, 2048], 12)):
        bw = range_model.BitWriter()
        range_model.put_alphabet(bw, [0, 1, 2])
        bw.put(4, 3)
        bw.put(width, 4)
        for f in freqs:
            bw.put(f - 1, width)
        bw.put(0, 200)
        cases.append((0, 5000, 0, bw.n, bw.bytes()))
        want.append("refused")
    got = run_cases(exe, tmp_path, cases)
    for (mode, count, start, bits, d), w, (err, used, out) in zip(cases, want, got):
        assert used <= bits
        if isinstance(w, bytes):
            assert err == 0 and out == w
        elif w == "short":
            assert err == 0 and len(out) < count
        else:
            assert err == 13, (count, bits)


def test_range_wide_frequency_emulated(tmp_path):
    """Chunks on which the reference's normalisation wraps a frequency to 0xFFFFFFFA (range_cases.WIDE): nobody can read them, but the
    reference writes them, with 64-bit cumulative products and with writeBits fields that are not masked inside a 64-bit word.
    k_range_stats marks such a chunk, k_range_encode_wide codes it and range_wide_spill adds the unmasked bits: the reference's bits
    (tests/golden/range.json, "wide"), alone and behind a chunk whose length puts it at 8 different positions in its word."""
    recs = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "range.json")))["wide"]["stage"]
    assert len(recs) == len(range_cases.WIDE) and len({r["bits"] % 64 for r in recs}) >= 8 and not any(r["ref_decodes"] for r in recs)
    blocks = [range_cases.make(r["recipe"]) for r in recs]
    for r, b in zip(recs, blocks):
        assert hashlib.md5(b).hexdigest() == r["input_md5"], r["recipe"]
    exe = build("range_emu", tmp_path, extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"])
    for order in ("0", "2"):
        got = run_cases(exe, tmp_path, [(1, 0, 0, 0, b) for b in blocks], order)
        for r, (err, bits, enc) in zip(recs, got):
            assert bits == r["bits"] and hashlib.md5(enc).hexdigest() == r["enc_md5"], (r["recipe"], order)
        # the decoder kernel refuses what the reference refuses
        back = run_cases(exe, tmp_path, [(0, len(b), 0, bits, enc) for b, (_, bits, enc) in zip(blocks, got)], order)
        for r, b, (err, _, out) in zip(recs, blocks, back):
            assert err != 0 or out != b, r["recipe"]
