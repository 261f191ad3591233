"""Writes tests/golden/pairs.json and tests/golden/pairs_typed.json from the reference build in oracle/_ref (build() makes it where the
reference sources exist).

Per case of tests/pair_cases.py (every ordered pair of the 14 device transforms, pass A in front of NONE, pass B in front of a rotation
of coders, checksum widths and job counts): chain, coder, checksum, jobs, length and md5 of the reference's .knz of the one input, and the
header's bit count, as one row per case in the order of the file's "fields" (a case left out has {"left_out": reason} behind its
settings instead). Settings, lengths and digests only.

Every case runs in a child process of its own, twice (MALLOC_PERTURB_=85 and =170): some chains make the reference write outside its
buffers, after which one process that ran them all dies much later in an unrelated case. A case is recorded as `left_out`, with the
reason, when the reference's call fails or its process dies, when it cannot read its own stream back to the input, or when its stream
differs between the two runs. At most pair_cases.MAX_LEFT_OUT cases per pass may be left out, and only chains whose second stage is
ZRLT (the BWT+ZRLT family of DESIGN.md section 4); otherwise the tool stops without writing a fixture that hides more.

pairs_typed.json is the same for the typed table of tests/pair_cases.py: the 93 ordered pairs of the 17 stages that hold EXE, TEXT or
DNA, over make_typed_input(). The reference writes, repeats and reads back every one of its cases, so it may leave out none.
    python tools/make_pair_golden.py [pairs] [typed]
"""
import concurrent.futures
import hashlib
import importlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


def child(path, chain, entropy, ck, jobs, bs):
    """One case in this process: what the reference wrote, and whether it reads it back."""
    d = open(path, "rb").read()
    ref = knzlib.Ref()
    rc, knz = ref.compress(d, chain, entropy, bs, jobs=jobs, checksum=ck, orig_size=len(d))
    out = {"rc": rc}
    if rc == 0:
        rc2, back = ref.decompress(knz, len(d) + bs, jobs=jobs)
        out.update({"knz_len": len(knz), "knz_md5": md5(knz), "head": knz[:32].hex(), "reads_back": int(rc2 == 0 and back == d)})
    print(json.dumps(out), flush=True)


def run_child(path, case, bs, perturb):
    chain, entropy, ck, jobs = case
    env = dict(os.environ, MALLOC_PERTURB_=str(perturb))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, chain, entropy, str(ck), str(jobs), str(bs)],
                       capture_output=True, text=True, env=env)
    lines = p.stdout.strip().splitlines()
    if p.returncode != 0 or not lines:
        return {"died": p.returncode}
    return json.loads(lines[-1])


def judge(a, b):
    """(record fields, None) or (None, reason for leaving the case out) from the two runs of a case."""
    for r in (a, b):
        if "died" in r:
            return None, "the reference's process died (exit status %d)" % r["died"]
        if r["rc"] != 0:
            return None, "the reference's call failed (code %d)" % r["rc"]
    if (a["knz_len"], a["knz_md5"]) != (b["knz_len"], b["knz_md5"]):
        return None, "the reference's stream differs between MALLOC_PERTURB_=85 and =170"
    if not (a["reads_back"] and b["reads_back"]):
        return None, "the reference cannot read its own stream back to the input"
    return a, None


def tables(cases):
    """name -> (fixture file, input, the cases in the file's row order as (pass, case), the left-out cases a pass may have, whether a
    left-out chain is of the allowed kind)"""
    pairs = [(i, j) for i in range(14) for j in range(14)]
    return {
        "pairs": ("pairs.json", cases.make_input, lambda ps: [cases.case(ps, i, j) for i, j in pairs],
                  cases.MAX_LEFT_OUT, lambda chain: chain.split("+")[1] == "ZRLT"),
        "typed": ("pairs_typed.json", cases.make_typed_input, lambda ps: [cases.case_typed(ps, i, j) for i, j in cases.typed_pairs()],
                  cases.MAX_LEFT_OUT_TYPED, lambda chain: False),
    }


def write_table(cases, framing, pool, name):
    """False when the table leaves out more than its condition allows (nothing is written then)"""
    fname, make, rows, max_left, allowed = tables(cases)[name]
    d = make()
    out = {"input_md5": md5(d), "n": len(d), "block_size": cases.BS, "passes": {},
           "fields": ["chain", "entropy", "checksum", "jobs", "knz_len", "knz_md5", "header_bits"]}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "input.bin")
        open(path, "wb").write(d)
        jobs = {ps: [[pool.submit(run_child, path, c, cases.BS, pb) for pb in (85, 170)] for c in rows(ps)] for ps in cases.PASSES}
        bad = False
        for ps in cases.PASSES:
            recs, left = [], []
            for (chain, entropy, ck, nj), runs in zip(rows(ps), jobs[ps]):
                got, reason = judge(*[f.result() for f in runs])
                if got is None:
                    recs.append([chain, entropy, ck, nj, {"left_out": reason}])
                    left.append(chain)
                    print("pass", ps, chain, entropy, "left out:", reason)
                else:
                    recs.append([chain, entropy, ck, nj, got["knz_len"], got["knz_md5"],
                                 framing.parse_header(bytes.fromhex(got["head"]))["bits"]])
            out["passes"][ps] = recs
            print("%s, pass %s: %d cases, %d left out" % (name, ps, len(recs), len(left)))
            if len(left) > max_left or not all(allowed(c) for c in left):
                print("pass %s leaves out more than the condition allows: %s" % (ps, left))
                bad = True
    if bad:
        return False
    path = os.path.join(ROOT, "tests", "golden", fname)
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")
    return True


def main(names):
    import pair_cases as cases
    knzlib.Ref()
    knzlib.load_pkg()
    framing = importlib.import_module("kanzi_amd.framing")
    names = names or list(tables(cases))
    if any(n not in tables(cases) for n in names):
        sys.exit("usage: make_pair_golden.py [%s]" % "|".join(tables(cases)))
    with concurrent.futures.ThreadPoolExecutor(max(1, min(16, (os.cpu_count() or 2) // 2))) as pool:
        ok = [write_table(cases, framing, pool, n) for n in names]
    if not all(ok):
        sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7]))
    else:
        main(sys.argv[1:])
