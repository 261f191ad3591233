"""Writes tests/golden/utf.json from the reference build in oracle/_ref (build() makes it where the reference sources exist).

Stage records: the recipe (tests/utf_cases.py), the data type the block comes with, the capacity (count + 8192), the reference's UTF
forward result (ok flag, data type afterwards, length, md5, the bytes in hex when short). The reference's TransformSequence gives a
stage a buffer of its own when the caller's is short, so the refusal of a destination below the bound is not recorded here (the tests
state it from UTFCodec.cpp:62). Inverse records: every accepted output decoded into len, len + 1 and len + 1000 bytes; the outputs of
utf_cases.DAMAGE_FROM damaged in the ways of utf_cases.DAMAGE, and random bytes, at three capacities each: the reference's verdict, and
its bytes when it accepts. Stream records: the md5 of the reference's headerless stream for each chain of utf_cases.STREAM_CHAINS, of
its .knz for utf_cases.HOSTED and the input of the CLI case. The reference gets output buffers at least 64 bytes larger than the
capacity it is told (knzlib.Ref: its inverse copies four bytes per symbol). The tests read only this file.
    python tools/make_utf_golden.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import utf_cases  # noqa: E402

SHORT = 96


def md5(b):
    return hashlib.md5(b).hexdigest()


def inv_record(ref, d, cap, **extra):
    ok, inv = ref.inverse("UTF", d, cap)
    rec = dict(extra, input_md5=md5(d), cap=cap, ok=int(ok == 1), inv_len=len(inv) if ok == 1 else None, inv_md5=md5(inv) if ok == 1 else None)
    if ok == 1 and len(inv) <= SHORT:
        rec["inv_hex"] = inv.hex()
    return rec


def main():
    ref = knzlib.Ref()
    out = {"stage": [], "inverse": [], "damaged": [], "streams": [], "hosted": [], "cli": None}
    outputs = []
    for r, dt in utf_cases.STAGE:
        d = utf_cases.make(r)
        cap = len(d) + 8192
        ok, fwd, dt_out = ref.forward_dt("UTF", d, cap, dt)
        rec = {"recipe": r, "dtype": dt, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1), "dtype_out": dt_out}
        if ok == 1:
            rec.update({"fwd_len": len(fwd), "fwd_md5": md5(fwd)})
            if len(fwd) <= SHORT:
                rec["fwd_hex"] = fwd.hex()
            lossy = r == utf_cases.LOSSY
            for cap2 in (len(d), len(d) + 1, len(d) + 1000) if len(d) else ():          # (an empty block takes no part in a batch)
                ir = inv_record(ref, fwd, cap2, stage=len(out["stage"]))
                if cap2 == len(d):
                    assert ir["ok"] == 0, r
                if cap2 > len(d):
                    assert ir["ok"] == 1 and (lossy or ir["inv_md5"] == md5(d)), r
                out["inverse"].append(ir)
        outputs.append(fwd if ok == 1 else None)
        out["stage"].append(rec)
    for i in utf_cases.DAMAGE_FROM:
        size = len(utf_cases.make(utf_cases.STAGE[i][0]))
        for op in utf_cases.DAMAGE:
            d = utf_cases.damage(outputs[i], op)
            for cap in (size, size + 1, size + 1000):
                out["damaged"].append(inv_record(ref, d, cap, stage=i, op=op))
    for r in utf_cases.INVERSE_RND:
        d = utf_cases.make(r)
        for cap in (len(d), 4 * len(d) + 1, 4 * len(d) + 1000):
            out["damaged"].append(inv_record(ref, d, cap, recipe=r))
    recs = out["inverse"] + out["damaged"]
    n_ok = sum(r["ok"] for r in recs)
    assert 3 * n_ok >= len(recs), (n_ok, len(recs))
    print("inverse records accepted by the reference: %d of %d" % (n_ok, len(recs)))
    d = utf_cases.make(utf_cases.STREAM)
    for chain, entropy, ck in utf_cases.STREAM_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, utf_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0, chain
        out["streams"].append({"chain": chain, "entropy": entropy, "block_size": utf_cases.STREAM_BS, "checksum": ck, "input_md5": md5(d),
                               "stream_len": len(enc), "stream_md5": md5(enc)})
    d = utf_cases.make(utf_cases.HOSTED_INPUT)
    for chain, entropy, bs, ck in utf_cases.HOSTED:
        for jobs in (1, 3):
            rc, enc = ref.compress(d, chain, entropy, bs, jobs=jobs, checksum=ck, orig_size=0)
            assert rc == 0, chain
            out["hosted"].append({"chain": chain, "entropy": entropy, "block_size": bs, "checksum": ck, "jobs": jobs,
                                  "input_md5": md5(d), "knz_md5": md5(enc), "knz_len": len(enc)})
    d = utf_cases.make(utf_cases.CLI)
    out["cli"] = {"recipe": utf_cases.CLI, "input_md5": md5(d)}
    path = os.path.join(ROOT, "tests", "golden", "utf.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path)
    for rec in out["stage"]:
        print(rec["recipe"][:3], rec["dtype"], rec["ok"], rec["dtype_out"], rec.get("fwd_len"))


if __name__ == "__main__":
    main()
