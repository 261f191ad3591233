"""Writes tests/golden/pack.json from the reference build in oracle/_ref (build() makes it where the reference sources exist).

Per-stage records: the recipe (tests/pack_cases.py), the reference's PACK forward result (ok flag, md5, the bytes in full when short) and
the result of its inverse on the forward output; inverse records: the reference's inverse of arbitrary bytes and of its own forward
outputs cut short. Stream records: the md5 of the reference's headerless stream for each chain of pack_cases.STREAM_CHAINS, and of
its .knz for the chains of pack_cases.HOSTED (TEXT / UTF on the host in front of PACK). The GPU tests read only this file.
    python tools/make_pack_golden.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import pack_cases  # noqa: E402

SHORT = 96


def md5(b):
    return hashlib.md5(b).hexdigest()


def main():
    ref = knzlib.Ref()
    out = {"stage": [], "inverse": [], "truncated": [], "streams": [], "hosted": []}
    for r in pack_cases.STAGE:
        d = pack_cases.make(r)
        cap = len(d) + 1024
        ok, fwd, _ = ref.forward("PACK", d, cap)
        rec = {"recipe": r, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1), "fwd_len": len(fwd), "fwd_md5": md5(fwd)}
        if len(fwd) <= SHORT:
            rec["fwd_hex"] = fwd.hex()
        if ok == 1:
            iok, back = ref.inverse("PACK", fwd, len(d))
            assert iok == 1 and back == d, r
        out["stage"].append(rec)
    for r in pack_cases.INVERSE:
        d = pack_cases.make(r)
        for cap in (len(d), 4 * len(d) + 64, 1 << 16):
            ok, inv = ref.inverse("PACK", d, cap)
            out["inverse"].append({"recipe": r, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1), "inv_md5": md5(inv) if ok == 1 else None})
    for r, cut in pack_cases.TRUNCATED:
        ok, fwd, _ = ref.forward("PACK", pack_cases.make(r), len(pack_cases.make(r)) + 1024)
        assert ok == 1, r
        d = fwd[:cut]
        for cap in (len(pack_cases.make(r)), 1 << 16):
            ok, inv = ref.inverse("PACK", d, cap)
            out["truncated"].append({"recipe": r, "cut": cut, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1),
                                     "inv_md5": md5(inv) if ok == 1 else None})
    for chain, entropy, bs, ck, r in pack_cases.HOSTED:
        d = pack_cases.make(r)
        rc, enc = ref.compress(d, chain, entropy, bs, jobs=1, checksum=ck, orig_size=0)
        assert rc == 0, chain
        out["hosted"].append({"chain": chain, "entropy": entropy, "block_size": bs, "checksum": ck, "recipe": r,
                              "input_md5": md5(d), "knz_md5": md5(enc), "knz_len": len(enc)})
    d = pack_cases.make(pack_cases.STREAM)
    for chain, entropy in pack_cases.STREAM_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, pack_cases.STREAM_BS, headerless=1)
        assert rc == 0, chain
        out["streams"].append({"chain": chain, "entropy": entropy, "block_size": pack_cases.STREAM_BS, "input_md5": md5(d),
                               "stream_len": len(enc), "stream_md5": md5(enc)})
    path = os.path.join(ROOT, "tests", "golden", "pack.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
