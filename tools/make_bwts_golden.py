"""Writes tests/golden/bwts.json from the reference build in oracle/_ref (build() makes it where the reference sources exist).

Per-stage records: the recipe (tests/bwts_cases.py), the md5 of the reference's BWTS forward output and of its inverse of the same bytes
read as a BWTS output (every byte string is one), both in full when short. Stream records: the recipe and the md5 of the reference's
.knz. The GPU and emulator tests read only this file.
    python tools/make_bwts_golden.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bwts_cases  # noqa: E402
import knzlib  # noqa: E402

SHORT = 64


def md5(b):
    return hashlib.md5(b).hexdigest()


def main():
    ref = knzlib.Ref()
    out = {"stage": [], "streams": [], "ranged": None, "big": None}
    for kind, recipes in (("stage", bwts_cases.STAGE), ("inverse", bwts_cases.INVERSE)):
        for r in recipes:
            d = bwts_cases.make(r)
            ok, fwd, _ = ref.forward("BWTS", d, len(d))
            assert ok, r
            ok, inv = ref.inverse("BWTS", d, len(d))
            assert ok, r
            rec = {"recipe": r, "kind": kind, "n": len(d), "input_md5": md5(d), "fwd_md5": md5(fwd), "inv_md5": md5(inv)}
            if len(d) <= SHORT:
                rec["fwd_hex"] = fwd.hex()
                rec["inv_hex"] = inv.hex()
            out["stage"].append(rec)
    for chain, entropy, bs, ck, r in bwts_cases.STREAMS:
        d = bwts_cases.make(r)
        rc, enc = ref.compress(d, chain, entropy, bs, jobs=1, checksum=ck, orig_size=0)
        assert rc == 0, (chain, entropy)
        out["streams"].append({"chain": chain, "entropy": entropy, "block_size": bs, "checksum": ck, "recipe": r, "n": len(d),
                               "input_md5": md5(d), "knz_md5": md5(enc), "knz_len": len(enc)})
    chain, entropy, bs, ck, r = bwts_cases.RANGED
    d = bwts_cases.make(r)
    rc, enc = ref.compress(d, chain, entropy, bs, jobs=1, checksum=ck, orig_size=len(d))
    assert rc == 0
    out["ranged"] = {"chain": chain, "entropy": entropy, "block_size": bs, "checksum": ck, "recipe": r, "n": len(d),
                     "input_md5": md5(d), "knz_md5": md5(enc), "knz_len": len(enc)}
    d = bwts_cases.make(bwts_cases.BIG)
    ok, fwd, _ = ref.forward("BWTS", d, len(d))
    assert ok
    out["big"] = {"recipe": bwts_cases.BIG, "n": len(d), "input_md5": md5(d), "fwd_md5": md5(fwd)}
    path = os.path.join(ROOT, "tests", "golden", "bwts.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
