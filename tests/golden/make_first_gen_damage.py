#!/usr/bin/env python3
"""Writes tests/golden/first_gen_damage.json: what the UNMODIFIED reference compiled into oracle/_ref/ (build container only) decides
on the damaged BWT and LZ / LZX blocks of tests/first_gen_damage.py:   make -C oracle ref && python tests/golden/make_first_gen_damage.py

Per case: accepted or refused, the length when accepted and the md5 of the bytes where they are defined. The file holds offsets and
values, never blocks.

What the reference cannot be asked, and what it does not define:
  * Its harness runs a transform through a TransformSequence, which wants a destination no shorter than its input. A capacity below
    that keeps the oracle's answer (source "oracle"); BWT.cpp:147-151 is the check the restatement makes there.
  * LZ: the reference reads its length extensions without looking for the end of the block (it asks for two readable bytes behind it,
    LZCodec.cpp:486-490). A damaged block can send it further. Every case is decoded with two bytes behind the block and with 4 KiB of
    zeros (what the restatement and the device read there); a case whose answers differ is taken out and listed under "dropped".
  * LZ: a match at distance 0 leaves the bytes the destination held. Every case is decoded into a destination of zeros and into one of
    0xA5; where decision or length differ the case is dropped, where only the bytes differ it keeps decision and length and has no md5.

The draw must test both sides: the reference accepts at least a quarter of the damaged LZ cases and refuses at least a quarter."""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import knzlib  # noqa: E402
import first_gen_damage as fgd  # noqa: E402


def ref_inverse(R, name, data, dst_cap, src_cap, fill):
    out = (C.c_uint8 * (dst_cap + 64))()
    C.memset(out, fill, dst_cap + 64)
    ol, sk = C.c_int(0), C.c_int(0)
    ok = R.L.ref_transform(name.encode(), 0, knzlib._buf(data), len(data), src_cap, out, dst_cap, b"", C.byref(ol), C.byref(sk))
    return (1, C.string_at(out, ol.value)) if ok == 1 else (0, b"")


def main():
    O, R = knzlib.Oracle(), knzlib.Ref()
    cases, dropped = [], []
    for rec in fgd.enumerate_cases(O):
        blk = fgd.block(O, rec)
        rec["intact"] = blk == fgd.encoded(O, rec)
        if rec["cap"] < len(blk):
            ok, out = O.inverse(rec["transform"], blk, rec["cap"])
            rec["source"] = "oracle"
            answers = [(1 if ok else 0, out if ok else b"")]
        elif rec["stage"] == "BWT":
            rec["source"] = "reference"
            answers = [ref_inverse(R, "BWT", blk, rec["cap"], 0, fill) for fill in (0, 0xA5)]
        else:
            rec["source"] = "reference"
            answers = [ref_inverse(R, rec["transform"], blk, rec["cap"], len(blk) + pad, fill) for pad in (2, 4096) for fill in (0, 0xA5)]
        if len({(ok, len(out)) for ok, out in answers}) != 1:
            rec["reason"] = "the reference's answer changes with the bytes behind the block or with what the destination held: " + \
                            ", ".join("%s %d" % ("accepts" if ok else "refuses", len(out)) for ok, out in answers)
            dropped.append(rec)
            continue
        ok, out = answers[0]
        rec["ok"] = ok
        if ok:
            rec["len"] = len(out)
            rec["md5"] = hashlib.md5(out).hexdigest() if len(set(out for _, out in answers)) == 1 else None
        cases.append(rec)
    lz = [r for r in cases if r["stage"] == "LZ" and not r["intact"]]
    acc = sum(r["ok"] for r in lz)
    print("LZ: %d damaged cases, %d accepted, %d refused, %d without md5; BWT: %d cases, %d accepted; dropped: %d" % (
        len(lz), acc, len(lz) - acc, sum(1 for r in lz if r["ok"] and r["md5"] is None),
        sum(1 for r in cases if r["stage"] == "BWT"), sum(r["ok"] for r in cases if r["stage"] == "BWT"), len(dropped)))
    for r in dropped:
        print("dropped:", r["transform"], r["input"], r["case"], r["damage"], r["cap"], r["reason"])
    assert 4 * acc >= len(lz) and 4 * (len(lz) - acc) >= len(lz), "the draw tests one side only"
    with open(fgd.PATH, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(r) for r in cases) + '\n],\n"dropped": [\n' + ",\n".join(json.dumps(r) for r in dropped) + "\n]}\n")


if __name__ == "__main__":
    main()
