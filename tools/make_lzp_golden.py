"""Writes tests/golden/lzp.json from the reference build in oracle/_ref (build() makes it where the reference sources exist).

Stage records: the recipe (tests/lzp_cases.py), the capacity, the reference's LZP forward result (ok flag, length, md5, the bytes in hex
when short); the reference's TransformSequence gives a stage a buffer of its own when the caller's is short, so the
refusal of a destination below the bound is not recorded here (the tests state it from LZCodec.cpp:788). Inverse records: the reference's inverse of bytes that are no LZP output at three capacities (one below the input length,
the decoded size, more), and of its own forward outputs cut inside a literal run, behind a match's 0xFC, inside a 0xFE run and in front
of the length byte, and whole into a destination one byte short. Stream records: the md5 of the reference's headerless stream for each chain of lzp_cases.STREAM_CHAINS, of its .knz
for lzp_cases.HOSTED and for the CLI case. The reference gets output buffers at least 64 bytes larger than the capacity it is told
(knzlib.Ref: its inverse may write 15 bytes past a match). The tests read only this file.
    python tools/make_lzp_golden.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import lzp_cases  # noqa: E402
import lzp_model  # noqa: E402

SHORT = 96


def md5(b):
    return hashlib.md5(b).hexdigest()


def inv_record(ref, d, cap, **extra):
    ok, inv = ref.inverse("LZP", d, cap)
    rec = dict(extra, input_md5=md5(d), cap=cap, ok=int(ok == 1), inv_md5=md5(inv) if ok == 1 else None)
    if ok == 1 and len(inv) <= SHORT:
        rec["inv_hex"] = inv.hex()
    return rec


def main():
    ref = knzlib.Ref()
    out = {"stage": [], "inverse": [], "cut": [], "streams": [], "hosted": [], "cli": None}
    for r in lzp_cases.STAGE:
        d = lzp_cases.make(r)
        for cap in (lzp_cases.max_encoded(len(d)),):
            ok, fwd, _ = ref.forward("LZP", d, cap)
            rec = {"recipe": r, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1)}
            if ok == 1:
                rec.update({"fwd_len": len(fwd), "fwd_md5": md5(fwd)})
                if len(fwd) <= SHORT:
                    rec["fwd_hex"] = fwd.hex()
                iok, back = ref.inverse("LZP", fwd, len(d))
                assert iok == 1 and back == d, r
            out["stage"].append(rec)
    for r in lzp_cases.INVERSE:
        d = lzp_cases.make(r)
        ok, inv = ref.inverse("LZP", d, 1 << 24)
        size = len(inv) if ok == 1 else len(d)
        for cap in (len(d) - 1, size, size + 1000):
            out["inverse"].append(inv_record(ref, d, cap, recipe=r))
    for r in lzp_cases.CUT_FROM:
        src = lzp_cases.make(r)
        ok, fwd, _ = ref.forward("LZP", src, lzp_cases.max_encoded(len(src)))
        assert ok == 1, r
        trace = []
        assert lzp_model.inverse(fwd, len(src), trace)[0]
        first = {}
        for kind, at in trace:
            if kind == "literal" and at < 6:
                continue
            first[kind] = at if kind == "literal" else first.get(kind, at)          # the last literal, the first match
        cuts = {"literal": first["literal"] + 1, "flag": first["flag"] + 1, "len": first["len"]}
        if "fe" in first:
            cuts["fe"] = first["fe"] + 1
        for kind, cut in sorted(cuts.items()):
            out["cut"].append(inv_record(ref, fwd[:cut], len(src), recipe=r, cut=cut, where=kind))
        # the whole output into a destination one byte short: the last literal, or the last match, does not fit
        out["cut"].append(inv_record(ref, fwd, len(src) - 1, recipe=r, cut=len(fwd), where="short"))
    recs = out["inverse"] + out["cut"]
    n_ok = sum(r["ok"] for r in recs)
    assert 3 * n_ok >= len(recs), (n_ok, len(recs))
    print("inverse records accepted by the reference: %d of %d" % (n_ok, len(recs)))
    d = lzp_cases.make(lzp_cases.STREAM)
    for chain, entropy, ck in lzp_cases.STREAM_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, lzp_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0, chain
        out["streams"].append({"chain": chain, "entropy": entropy, "block_size": lzp_cases.STREAM_BS, "checksum": ck, "input_md5": md5(d),
                               "stream_len": len(enc), "stream_md5": md5(enc)})
    for chain, entropy, bs, ck, r in lzp_cases.HOSTED:
        d = lzp_cases.make(r)
        for jobs in (1, 3):
            rc, enc = ref.compress(d, chain, entropy, bs, jobs=jobs, checksum=ck, orig_size=0)
            assert rc == 0, chain
            out["hosted"].append({"chain": chain, "entropy": entropy, "block_size": bs, "checksum": ck, "jobs": jobs, "recipe": r,
                                  "input_md5": md5(d), "knz_md5": md5(enc), "knz_len": len(enc)})
    d = lzp_cases.make(lzp_cases.CLI)
    out["cli"] = {"recipe": lzp_cases.CLI, "input_md5": md5(d)}
    path = os.path.join(ROOT, "tests", "golden", "lzp.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path)
    for rec in out["stage"]:
        print(rec["recipe"][:3], rec["cap"], rec["ok"], rec.get("fwd_len"))


if __name__ == "__main__":
    main()
