"""Writes tests/golden/newer_cross.json from the reference build in oracle/_ref (build() makes it where the reference sources exist).

Per chain of tests/newer_cross_cases.py: length and md5 of the reference's .knz of the one input (with the chain's jobs and checksum), and
for each seeded damaged copy of that stream whether the reference's decompressor accepted it and, if so, length and md5 of what it
returned. Recipes, lengths, flags and digests only.
    python tools/make_newer_cross_golden.py
"""
import hashlib
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import newer_cross_cases as cases  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


def main():
    ref = knzlib.Ref()
    knzlib.load_pkg()
    framing = importlib.import_module("kanzi_amd.framing")
    d = cases.make_input()
    out = {"input_md5": md5(d), "n": len(d), "block_size": cases.BS, "chains": []}
    for idx, (chain, entropy, ck, jobs) in enumerate(cases.CHAINS):
        rc, knz = ref.compress(d, chain, entropy, cases.BS, jobs=jobs, checksum=ck, orig_size=len(d))
        assert rc == 0, chain
        rc, back = ref.decompress(knz, len(d) + cases.BS, jobs=jobs)
        assert rc == 0 and back == d, chain
        hdr_bits = framing.parse_header(knz)["bits"]
        first = (hdr_bits + 7) // 8
        rec = {"chain": chain, "entropy": entropy, "checksum": ck, "jobs": jobs, "knz_len": len(knz), "knz_md5": md5(knz),
               "header_bits": hdr_bits, "damaged": []}
        for v in range(cases.VARIANTS):
            bad = cases.damage(knz, first, idx, v)
            rc, got = ref.decompress(bad, len(d) + cases.BS, jobs=jobs)
            rec["damaged"].append({"variant": v, "input_len": len(bad), "input_md5": md5(bad), "accepted": int(rc == 0),
                                   "out_len": len(got) if rc == 0 else 0, "out_md5": md5(got) if rc == 0 else None})
        out["chains"].append(rec)
        print(chain, entropy, len(knz), [r["accepted"] for r in rec["damaged"]])
    path = os.path.join(ROOT, "tests", "golden", "newer_cross.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
