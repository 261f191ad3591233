"""Writes tests/golden/mm.json from the reference build in oracle/_ref (build() makes it where the reference sources exist).

Per-stage records: the recipe (tests/mm_cases.py), the reference's MM forward result (ok flag, length, md5, the bytes in full when short),
its mode and distance; inverse records: the reference's inverse of arbitrary and header-shaped bytes and of its own forward outputs cut
short, at two capacities. Stream records: the md5 of the reference's headerless stream for each chain of mm_cases.STREAM_CHAINS, and of
its .knz for mm_cases.HOSTED. The GPU and emulator tests read only this file.
The "finalfail" records fail ONLY the forward's final check (FSDCodec.cpp:273-286): a walk inside a band of 32 values with noise in tenth 4
(XOR coding, so no overflow) is accepted by the reference; the same bytes with noise also in tenths 2 and 6, which nothing but the final
check reads, are refused. main() asserts both halves.
    python tools/make_mm_golden.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import mm_cases  # noqa: E402

SHORT = 96


def md5(b):
    return hashlib.md5(b).hexdigest()


def main():
    ref = knzlib.Ref()
    out = {"stage": [], "inverse": [], "truncated": [], "streams": [], "hosted": []}
    for r in mm_cases.STAGE:
        d = mm_cases.make(r)
        cap = mm_cases.max_encoded(len(d))
        ok, fwd, _ = ref.forward("MM", d, cap)
        rec = {"recipe": r, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1)}
        if ok == 1:
            rec.update({"fwd_len": len(fwd), "fwd_md5": md5(fwd), "mode": fwd[0], "dist": fwd[1]})
            iok, back = ref.inverse("MM", fwd, cap)
            assert iok == 1 and back == d, r
        out["stage"].append(rec)
    for r in mm_cases.STAGE:
        if r[0] != "finalfail":
            continue
        d = bytearray(mm_cases.make(r))
        assert ref.forward("MM", bytes(d), mm_cases.max_encoded(len(d)))[0] != 1, r
        t = len(d) // 10
        for k in (2, 6):                     # tenth 1 has the same band walk: without the noise the block is accepted, in XOR mode
            d[k * t:(k + 1) * t] = d[t:2 * t]
        ok, fwd, _ = ref.forward("MM", bytes(d), mm_cases.max_encoded(len(d)))
        assert ok == 1 and fwd[0] == 1, r
    n_ok = 0
    for r in mm_cases.INVERSE:
        d = mm_cases.make(r)
        for cap in (len(d), len(d) + (1 << 16)):
            ok, inv = ref.inverse("MM", d, cap)
            n_ok += ok == 1
            rec = {"recipe": r, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1), "inv_md5": md5(inv) if ok == 1 else None}
            if ok == 1 and len(inv) <= SHORT:
                rec["inv_hex"] = inv.hex()
            out["inverse"].append(rec)
    for r, cut in mm_cases.TRUNCATED:
        src = mm_cases.make(r)
        ok, fwd, _ = ref.forward("MM", src, mm_cases.max_encoded(len(src)))
        assert ok == 1, r
        d = fwd[:cut]
        for cap in (cut, mm_cases.max_encoded(len(src))):
            ok, inv = ref.inverse("MM", d, cap)
            n_ok += ok == 1
            out["truncated"].append({"recipe": r, "cut": cut, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1),
                                     "inv_md5": md5(inv) if ok == 1 else None})
    total = len(out["inverse"]) + len(out["truncated"])
    assert 2 * n_ok >= total, (n_ok, total)
    print("inverse records accepted by the reference: %d of %d" % (n_ok, total))
    for chain, entropy, bs, ck, r in mm_cases.HOSTED:
        d = mm_cases.make(r)
        rc, enc = ref.compress(d, chain, entropy, bs, jobs=1, checksum=ck, orig_size=0)
        assert rc == 0, chain
        out["hosted"].append({"chain": chain, "entropy": entropy, "block_size": bs, "checksum": ck, "recipe": r,
                              "input_md5": md5(d), "knz_md5": md5(enc), "knz_len": len(enc)})
    d = mm_cases.make(mm_cases.STREAM)
    for chain, entropy in mm_cases.STREAM_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, mm_cases.STREAM_BS, headerless=1)
        assert rc == 0, chain
        out["streams"].append({"chain": chain, "entropy": entropy, "block_size": mm_cases.STREAM_BS, "input_md5": md5(d),
                               "stream_len": len(enc), "stream_md5": md5(enc)})
    path = os.path.join(ROOT, "tests", "golden", "mm.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path)
    for rec in out["stage"]:
        print(rec["recipe"][:5], rec["ok"], rec.get("mode"), rec.get("dist"), rec.get("fwd_len"))


if __name__ == "__main__":
    main()
