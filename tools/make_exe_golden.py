"""Writes tests/golden/exe.json from the reference build in oracle/_ref (build() makes it where the reference sources exist).

Stage records: the recipe (tests/exe_cases.py), its name, the data type the block comes with, the capacity (getMaxEncodedLength), the
reference's EXE forward result (ok flag, data type afterwards, length, md5) and what its inverse makes of that (ARM64 code that does
not start at a multiple of 4 does not come back: the forward drops two bits of every target). The reference's TransformSequence gives
a stage a buffer of its own when the caller's is short, so the refusal of a destination below the bound is not recorded here (the tests state it from
EXECodec.cpp:77). Damaged records: the outputs of exe_cases.DAMAGE_FROM damaged in the ways of exe_cases.DAMAGE, decoded into the
encoded length (the least the sequence lets through) and into getMaxEncodedLength of the original: the reference's verdict, and its
bytes when it accepts. Stream records: the md5 of the reference's headerless stream for the ragged batch and each chain of
exe_cases.STREAM_CHAINS, of its .knz for exe_cases.HOSTED, and the input of the CLI case. No input bytes are stored; the tests read
only this file. The tool fails when the reference does not give a record of exe_cases.REQUIRED the verdict stated there, when a whole
record is refused or when no damaged record is.
    python tools/make_exe_golden.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exe_cases  # noqa: E402
import knzlib  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


def build_golden(log=print):
    """Every record, from the reference (tests/test_exe_golden.py compares the stored file with this)."""
    ref = knzlib.Ref()
    out = {"stage": [], "damaged": [], "streams": [], "hosted": [], "ragged": None, "cli": None}
    fwd_of, seen = {}, set()
    for r, dt, name in exe_cases.STAGE:
        d = exe_cases.make(r)
        cap = exe_cases.max_encoded(len(d))
        ok, fwd, dt_out = ref.forward_dt("EXE", d, cap, dt)
        rec = {"name": name, "recipe": r, "dtype": dt, "input_md5": md5(d), "cap": cap, "ok": int(ok == 1), "dtype_out": dt_out}
        if ok == 1:
            ok2, inv = ref.inverse("EXE", fwd, len(fwd))
            assert ok2 == 1, name
            rec.update({"fwd_len": len(fwd), "fwd_md5": md5(fwd), "mode": fwd[0], "inv_md5": md5(inv), "lossless": int(inv == d)})
            if inv != d:
                log("the reference does not give this block back:", name)
            fwd_of[name] = (d, fwd)
        if name in exe_cases.REQUIRED:
            assert (rec["ok"], dt_out) == exe_cases.REQUIRED[name], (name, rec["ok"], dt_out)
            seen.add(name)
        log("%-50s ok %d type %d -> %d %s" % (name, rec["ok"], dt, dt_out, (len(d), len(fwd)) if ok == 1 else ""))
        out["stage"].append(rec)
    assert seen == set(exe_cases.REQUIRED), set(exe_cases.REQUIRED) - seen
    # the first count of escape pairs that a block of 4,096 bytes cannot afford lies inside the counts tried
    below = [(int(n.split()[1]), fwd_of.get(n) is not None) for _, _, n in exe_cases.STAGE if n.endswith("below 0")]
    assert below[0][1] and not below[-1][1] and any(a[1] and not b[1] and b[0] == a[0] + 1 for a, b in zip(below, below[1:])), below
    n_refused = 0
    for name in exe_cases.DAMAGE_FROM:
        d, fwd = fwd_of[name]
        for op in exe_cases.DAMAGE:
            bad = exe_cases.damage(fwd, op)
            if bad is None:
                continue
            for cap in (len(bad), exe_cases.max_encoded(len(d))):
                ok, inv = ref.inverse("EXE", bad, cap)
                if op == "whole":
                    assert ok == 1 and inv == d, (name, cap)
                n_refused += ok != 1
                out["damaged"].append({"stage": name, "op": op, "input_md5": md5(bad), "cap": cap, "ok": int(ok == 1),
                                       "inv_len": len(inv) if ok == 1 else None, "inv_md5": md5(inv) if ok == 1 else None})
    assert n_refused > 0
    assert {"escend", "armhalf"} <= {r["op"] for r in out["damaged"]}
    log("damaged records: %d, refused %d" % (len(out["damaged"]), n_refused))
    d = exe_cases.make(exe_cases.RAGGED)
    rc, enc = ref.compress(d, "EXE", "NONE", exe_cases.RAGGED_BS, headerless=1)
    assert rc == 0
    rc, plain = ref.compress(d, "NONE", "NONE", exe_cases.RAGGED_BS, headerless=1)
    assert rc == 0 and len(enc) != len(plain), "EXE took no block of the ragged batch"
    out["ragged"] = {"block_size": exe_cases.RAGGED_BS, "input_md5": md5(d), "stream_len": len(enc), "stream_md5": md5(enc)}
    d = exe_cases.make(exe_cases.STREAM)
    for chain, entropy, ck in exe_cases.STREAM_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, exe_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0, chain
        log(chain, entropy, len(enc))
        out["streams"].append({"chain": chain, "entropy": entropy, "block_size": exe_cases.STREAM_BS, "checksum": ck, "input_md5": md5(d),
                               "stream_len": len(enc), "stream_md5": md5(enc)})
    for chain, entropy, bs, ck in exe_cases.HOSTED:
        for jobs in (1, 3):
            rc, enc = ref.compress(d, chain, entropy, bs, jobs=jobs, checksum=ck, orig_size=0)
            assert rc == 0, chain
            rc, back = ref.decompress(enc, len(d) + bs, jobs)
            assert rc == 0 and back == d, chain
            out["hosted"].append({"chain": chain, "entropy": entropy, "block_size": bs, "checksum": ck, "jobs": jobs,
                                  "input_md5": md5(d), "knz_md5": md5(enc), "knz_len": len(enc)})
    d = exe_cases.make(exe_cases.CLI)
    out["cli"] = {"recipe": exe_cases.CLI, "input_md5": md5(d)}
    return json.loads(json.dumps(out))


def main():
    out = build_golden()
    path = os.path.join(ROOT, "tests", "golden", "exe.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
