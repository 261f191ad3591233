"""Writes tests/golden/rolzx.json: recipes (tests/rolzx_cases.py), lengths and md5s, no input bytes.

The reference harness's per-stage entry point does not reach ROLZCodec2 (it never puts "transform" into the Context, so ROLZCodec builds
ROLZCodec1 for either name). Stage records therefore come from tests/rolzx_model.py, which tests/test_rolzx_model.py pins to the
reference through `kanzi -t ROLZX -e NONE`; this tool repeats that check for every accepted record before it writes one. Stream, hosted,
CLI and chunk records (16 MiB and more) come from the reference build in oracle/_ref itself.
  stage    forward of rolzx_cases.STAGE with an UNDEFINED type and of rolzx_cases.PRESET with a preset one: verdict, length, md5, type left
  damaged  inverse of forward outputs whole, cut (inside the first literals, mid-stream, 1 to 4 bytes before the end), with a byte
           flipped and with a length field above the capacity: the model's verdict and bytes. Asserted: every whole record is accepted,
           some damaged record is refused, and none ends where the reference would write outside its buffers
  ragged   71 blocks of 4,096 bytes that mix the stage records' kinds through ROLZX / NONE: the reference's stream
  chunks   blocks of 16 MiB and a little more through ROLZX / NONE at 32 MiB blocks: the reference's stream and what it decodes it to
    python tools/make_rolzx_golden.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knzlib  # noqa: E402
import rolzx_cases  # noqa: E402
import rolzx_model  # noqa: E402


def md5(b):
    return hashlib.md5(b).hexdigest()


def bits(b):
    return "".join(format(x, "08b") for x in b)


def in_reference_stream(d, out, tmp):
    """The model's stage output as a bit string inside the reference's `-t ROLZX -e NONE` file of d (the block header is not byte-aligned)"""
    src, knz = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.knz")
    open(src, "wb").write(d)
    p = subprocess.run([knzlib.REF_BIN, "-c", "-i", src, "-o", knz, "-f", "-t", "ROLZX", "-e", "NONE", "-j", "1"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return bits(out) in bits(open(knz, "rb").read())


def main():
    ref = knzlib.Ref()
    out = {"stage": [], "damaged": [], "chunks": [], "streams": [], "hosted": [], "cli": None}
    tmp = tempfile.mkdtemp()
    fwd_of = {}
    for r, dt_in in [(r, 0) for r in rolzx_cases.STAGE] + [(r, t) for r, t in rolzx_cases.PRESET]:
        d = rolzx_cases.make(r)
        cap = rolzx_cases.max_encoded(len(d))
        ok, fwd, dt_out, _ = rolzx_model.forward(d, cap, dt_in)
        rec = {"recipe": r, "input_md5": md5(d), "cap": cap, "dtype_in": dt_in, "ok": int(ok), "dtype_out": dt_out}
        if ok and d:
            rec.update({"fwd_len": len(fwd), "fwd_md5": md5(fwd)})
            iok, back, _ = rolzx_model.inverse(fwd, len(d))
            assert iok and back == d, r
            # what a stream does with the block: the type from its magic (ELF), no preset otherwise
            if dt_in == (3 if r[0] == "elf" else 0):
                assert in_reference_stream(d, fwd, tmp), ("the model's output is not in the reference's stream", r)
            if dt_in == 0:
                fwd_of[json.dumps(r)] = fwd
        out["stage"].append(rec)
    n_refused = 0
    for r in rolzx_cases.CUT_FROM:
        d = rolzx_cases.make(r)
        fwd = fwd_of[json.dumps(r)]
        n = len(fwd)
        ops = [["whole"]] + [["cut", k] for k in (4, 9, 12, 13, 15, n // 2, n - 4, n - 3, n - 2, n - 1)] \
            + [["flip", k, x] for k, x in ((4, 4), (5, 0x80), (14, 1), (n // 2, 0x10), (n - 9, 1), (n - 1, 0xFF))] + [["len", 1], ["len", -1], ["len", 1 << 20]]
        for op in ops:
            bad = rolzx_cases.damage(fwd, op)
            for cap in (len(d),) + ((len(d) + 100,) if op[0] == "len" else ()):
                ok, inv, paths = rolzx_model.inverse(bad, cap)
                if "refuse_write_outside" in paths:
                    print("dropped (the reference would write outside its buffers):", r[:3], op)
                    continue
                assert ok or op[0] != "whole", r
                n_refused += 0 if ok else 1
                out["damaged"].append({"recipe": r, "op": op, "input_md5": md5(bad), "cap": cap, "ok": int(ok), "inv_md5": md5(inv) if ok else None})
    assert n_refused > 0
    print("damaged records: %d, refused %d" % (len(out["damaged"]), n_refused))
    bs = 32 << 20
    for r in rolzx_cases.CHUNKS:
        d = rolzx_cases.make(r)
        rc, enc = ref.compress(d, "ROLZX", "NONE", bs, headerless=1)
        assert rc == 0, r
        assert len(enc) < len(d) // 4, "ROLZX took the block"
        rec = {"recipe": r, "input_md5": md5(d), "block_size": bs, "stream_len": len(enc), "stream_md5": md5(enc)}
        # the reference's own verdict on its own stream, through its command-line tool (16 MiB + 1 to + 11: it cannot decode it)
        src, knz, dec = (os.path.join(tmp, n) for n in ("c.bin", "c.knz", "c.out"))
        open(src, "wb").write(d)
        p = subprocess.run([knzlib.REF_BIN, "-c", "-i", src, "-o", knz, "-f", "-t", "ROLZX", "-e", "NONE", "-b", "32m", "-j", "1"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        if os.path.exists(dec):
            os.remove(dec)
        p = subprocess.run([knzlib.REF_BIN, "-d", "-i", knz, "-o", dec, "-f", "-j", "1"], capture_output=True, text=True)
        good = p.returncode == 0 and os.path.exists(dec) and open(dec, "rb").read() == d
        rec["reference_decodes_it"] = int(good)
        print(r[:2], "stream", len(enc), "reference decodes its own output:", good)
        out["chunks"].append(rec)
    d = rolzx_cases.make(rolzx_cases.STREAM)
    for chain, entropy, ck in rolzx_cases.STREAM_CHAINS:
        rc, enc = ref.compress(d, chain, entropy, rolzx_cases.STREAM_BS, headerless=1, checksum=ck)
        assert rc == 0, chain
        out["streams"].append({"chain": chain, "entropy": entropy, "block_size": rolzx_cases.STREAM_BS, "checksum": ck, "input_md5": md5(d),
                               "stream_len": len(enc), "stream_md5": md5(enc)})
    d = rolzx_cases.make(rolzx_cases.RAGGED)
    rc, enc = ref.compress(d, "ROLZX", "NONE", rolzx_cases.RAGGED_BS, headerless=1)
    assert rc == 0
    out["ragged"] = {"block_size": rolzx_cases.RAGGED_BS, "input_md5": md5(d), "stream_len": len(enc), "stream_md5": md5(enc)}
    for chain, entropy, bsz, ck, r in rolzx_cases.HOSTED:
        d = rolzx_cases.make(r)
        for jobs in (1, 3):
            rc, enc = ref.compress(d, chain, entropy, bsz, jobs=jobs, checksum=ck, orig_size=0)
            assert rc == 0, chain
            out["hosted"].append({"chain": chain, "entropy": entropy, "block_size": bsz, "checksum": ck, "jobs": jobs, "recipe": r,
                                  "input_md5": md5(d), "knz_md5": md5(enc), "knz_len": len(enc)})
    d = rolzx_cases.make(rolzx_cases.CLI)
    out["cli"] = {"recipe": rolzx_cases.CLI, "input_md5": md5(d)}
    path = os.path.join(ROOT, "tests", "golden", "rolzx.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
