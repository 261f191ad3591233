"""Writes tests/golden/pack.json from the reference build in oracle/_ref (build() makes it where the reference sources exist).

Per-stage records: the recipe (tests/pack_cases.py), the reference's PACK forward result (ok flag, md5, the bytes in full when
short, the Context's data type afterwards) and the result of its inverse on the forward output.
Preset records: the forward result of one ACGT block under every data type of pack_cases.PRESET_TYPES.
Inverse records: the reference's inverse of arbitrary bytes and of its own forward outputs cut short.
Damaged records (pack_cases.DAMAGED): the reference's inverse of seeded header-shaped bytes and of its forward outputs with a few
header bytes overwritten. Every capacity is at least the input's length: below that TransformSequence::inverse refuses before
AliasCodec is asked, and the record would hold the sequence's verdict.
Stream records: the md5 of the reference's headerless stream for each chain of pack_cases.STREAM_CHAINS, and of its .knz for the
chains of pack_cases.HOSTED (TEXT / UTF on the host in front of PACK). The tests read only this file.
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
    out = {"stage": [], "inverse": [], "truncated": [], "presets": [], "damaged": [], "streams": [], "hosted": []}
    for r in pack_cases.STAGE:
        d = pack_cases.make(r)
        cap = len(d) + 1024
        ok, fwd, _ = ref.forward("PACK", d, cap)
        ok2, fwd2, dt_after = ref.forward_dt("PACK", d, cap)
        assert ok2 == ok and (ok != 1 or fwd2 == fwd), r
        rec = {"recipe": r, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1), "fwd_len": len(fwd), "fwd_md5": md5(fwd),
               "dt_after": dt_after}
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
    d = pack_cases.make(pack_cases.PRESET_BLOCK)
    for dt in pack_cases.PRESET_TYPES:
        ok, fwd, dt_after = ref.forward_dt("PACK", d, len(d) + 1024, dt)
        out["presets"].append({"dt": dt, "ok": int(ok == 1), "dt_after": dt_after, "fwd_md5": md5(fwd) if ok == 1 else None})
    assert len(pack_cases.DAMAGED) <= 100
    for r in pack_cases.DAMAGED:
        if r[0] == "overwrite":
            src = pack_cases.make(r[3])
            ok, fwd, _ = ref.forward("PACK", src, len(src) + 1024)
            assert ok == 1, r
            d = pack_cases.overwrite(fwd, r[2], r[4])
        else:
            d = pack_cases.make(r)
        cap = max(4 * len(d) + 64, pack_cases.DAMAGED_CAP_MIN)
        assert cap >= len(d)
        ok, inv = ref.inverse("PACK", d, cap)
        out["damaged"].append({"recipe": r, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1), "inv_len": len(inv) if ok == 1 else 0,
                               "inv_md5": md5(inv) if ok == 1 else None})
    n_acc = sum(r["ok"] for r in out["damaged"])
    assert 2 * n_acc >= len(out["damaged"]), (n_acc, len(out["damaged"]))     # tests/test_emu_pack.py asks for at least half
    print("damaged:", len(out["damaged"]), "records,", n_acc, "accepted by the reference")
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
