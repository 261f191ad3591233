"""The damaged BWT and LZ / LZX blocks of tests/golden/first_gen_damage.json: which cases there are (drawn from bwt_inverse_cases and
lz_decoder_cases), and how a record of the fixture becomes the block it stands for. The fixture holds offsets and values only; the
blocks are the oracle's encodings of generated inputs.

A record: stage ("BWT" / "LZ"), transform, bs_version, input (a vectors.make spec, or ["lz_block", name]), case (a label), damage
([[offset, value], ...]), cut (length the block is cut to), cap (destination capacity), and -- written by the generator
tests/golden/make_first_gen_damage.py -- source ("reference", or "oracle" where the reference's harness cannot be asked: a destination
shorter than the input), ok, len (when accepted), md5 (when accepted and the bytes are defined), intact (the block is as encoded)."""
import json
import os

import bwt_inverse_cases
import lz_decoder_cases
import vectors

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_gen_damage.json")

# LZX, text(60000, 3), nDist + 47: the disagreement between oracle/lz.c and the reference that the fixture was first drawn up for (see
# tests/test_oracle_vs_ref.py::test_lzx_extensions_read_behind_the_block)
LZ_EXTRA = {("text", "LZX"): (("nDist+47", ((8, 183),)),)}

_enc = {}


def plain(rec):
    spec = rec["input"]
    return lz_decoder_cases.blocks()[spec[1]] if spec[0] == "lz_block" else vectors.make(tuple(spec))


def encoded(oracle, rec):
    """The oracle's encoding of the record's input (bitstream version 6)."""
    key = (rec["transform"], tuple(rec["input"]))
    if key not in _enc:
        d = plain(rec)
        cap = len(d) + 64 if rec["stage"] == "BWT" else lz_decoder_cases.forward_cap(len(d))
        ok, enc = oracle.forward(rec["transform"], d, cap)
        assert ok, key
        _enc[key] = enc
    return _enc[key]


def block(oracle, rec):
    b = bytearray(encoded(oracle, rec))
    for off, v in rec["damage"]:
        b[off] = v
    return bytes(b[:rec["cut"]])


def enumerate_cases(oracle):
    """Every case, without results, in the fixture's order."""
    out = []
    for spec in bwt_inverse_cases.HEADER_SPECS:
        rec0 = {"stage": "BWT", "transform": "BWT", "bs_version": 6, "input": list(spec)}
        enc = encoded(oracle, rec0)
        for i, (damage, cut, cap) in enumerate(bwt_inverse_cases.header_damage(enc, spec[1])):
            out.append(dict(rec0, case="header %d" % i, damage=[list(x) for x in damage], cut=cut, cap=cap))
    for name, data in lz_decoder_cases.blocks().items():
        if name == "tiny":
            continue                                    # (the forward transform refuses it: there is no block to damage)
        for t in lz_decoder_cases.TRANSFORMS:
            rec0 = {"stage": "LZ", "transform": t, "bs_version": 6, "input": ["lz_block", name]}
            enc = encoded(oracle, rec0)
            lz_decoder_cases.check(name, enc)
            for sec, damage in tuple(lz_decoder_cases.damage_cases(name, t, enc)) + LZ_EXTRA.get((name, t), ()):
                for cap in (len(data), len(data) + 64):
                    out.append(dict(rec0, case=sec, damage=[list(x) for x in damage], cut=len(enc), cap=cap))
    return out


def key(rec):
    return (rec["stage"], rec["transform"], tuple(rec["input"]), rec["case"], tuple(map(tuple, rec["damage"])), rec["cut"], rec["cap"])


def load():
    """(cases, dropped) of the committed fixture."""
    f = json.load(open(PATH))
    return f["cases"], f["dropped"]
