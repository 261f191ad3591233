"""Randomised parity soak: random chains / codecs / block sizes / inputs / jobs / checksums, device stream vs expected stream and
device decode of the expected stream (developer tool).   usage: gpu_soak.py SEED SECONDS [first|newer]

first (the default; tests/test_gpu_parity.py::test_randomised_soak): the 16 chains and 5 coders of the first generation, expected
streams from the C oracle.

newer (test_randomised_soak_newer_stages): the same draw over those tables plus the chains of NEWER_CHAINS (BWTS, PACK, MM, LZP, ROLZX,
UTF, EXE, TEXT and DNA alone, in front of and behind first-generation stages, and two of them in one chain) and the coders RANGE, CM, TPAQ and TPAQX. A case whose chain
and coder the oracle knows stays on the oracle; any other takes its expected stream from the reference build (knzlib.Ref,
oracle/_ref/libkanzi_ref.so) with the same jobs and checksum, and where that build is absent the case is skipped and counted. The
input kinds grow by six that the newer stages accept: four at every block size from 4,096 up (checked with Ref.forward at 4,096, 65,536,
262,144 and 1 MiB): `walk` (a bounded random walk: MM, and PACK in its digram mode), `alpha12` and `acgt` (12 skewed symbols and
ACGT: PACK's digram and 2-bit modes) and `repeats` (corpus.repeats, text with copied spans of 1 KiB and more: LZP, and PACK), and
`utf8` (utf_cases.utf8, code points of one byte and more, cut wherever a block ends: UTF), and `x86` (exe_cases.x86, instruction-like
bytes with relative jumps: EXE from 4,096 up). EXE, TEXT and DNA are device stages; the pair matrix holds them at 16 KiB only, and TEXT's
scratch and EXE's scan tiles depend on the block size, which this draw varies. Their 13 chains (EXE, EXE+ROLZX, EXE+PACK+ZRLT,
EXE+BWT+RANK+ZRLT, MM+EXE, TEXT, TEXT+UTF+BWT+RANK+ZRLT, TEXT+PACK, TEXT+ROLZX, LZP+TEXT, EXE+TEXT, DNA, DNA+RLT) were run through
knzlib.Ref alone over all twelve input kinds at the five block sizes, with NONE, HUFFMAN, ANS0 and TPAQ, 1 to 8 jobs and every checksum
width: the reference read back every stream it wrote, so none of them was dropped. Of the
older kinds MM also takes `runs`, LZP `mixed`, `runs` and `sparse`, PACK `text` and `small_alpha` at all four sizes.
CM, TPAQ, TPAQX and FPAQ code one block per wave (CM at 2.85 us per byte): n is capped at 65,536 for CM, TPAQ and TPAQX
and at 300,000 for FPAQ. The three binary coders get the output buffer of their second tier (knz_hip_encode_bound is their first).

Left out in both: BWT+ZRLT and BWT+RLT+ZRLT, and chains that start with ZRLT / RLT / SRT on `rand`; LZ and LZX
behind PACK, MM, UTF or ROLZX (the device refuses to write those chains by design; tests/test_gpu_pairs.py has it read the
reference's) and behind EXE, TEXT or DNA (the same refusal); TIMESTAMP, which has no name at the stream level; block sizes above 1 MiB (the per-stage tests and tests/test_emu_pack.py hold
the larger blocks). Every ordered pair of the device transforms, which this draw only samples, is in tests/test_gpu_pairs.py."""
import sys, os, time, importlib
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import knzlib, vectors, utf_cases, exe_cases
import numpy as np

# chains whose even-indexed stages cannot expand into the caller's buffer
# (BWT+ZRLT and BWT+RLT+ZRLT are left out: with a skipped or expanding second stage the reference writes streams
# that it cannot decode itself -- checked with oracle/_ref -- so there is nothing to be bit-exact with)
CHAINS = ["NONE", "BWT", "BWT+MTFT+ZRLT", "BWT+SRT+ZRLT", "BWT+MTFT", "RLT", "ZRLT", "SRT", "RLT+ZRLT", "MTFT", "BWT+SRT", "LZ", "LZX", "RLT+LZX", "RANK", "BWT+RANK+ZRLT"]
ENTS = ["NONE", "ANS0", "ANS1", "HUFFMAN", "FPAQ"]
KINDS = ["text", "mixed", "rand", "runs", "sparse", "small_alpha"]
NEWER_CHAINS = ["BWTS", "BWTS+MTFT+ZRLT", "BWTS+SRT+ZRLT", "PACK", "PACK+BWT+MTFT+ZRLT", "PACK+RLT", "PACK+MM", "MM", "MM+PACK", "MM+RLT",
                "MM+BWT+MTFT+ZRLT", "LZP", "LZP+BWT+RANK+ZRLT", "BWT+LZP", "LZP+LZX", "LZP+BWTS+MTFT+ZRLT", "PACK+LZP", "LZP+BWT+LZP",
                "ROLZX", "PACK+ROLZX", "ROLZX+RLT", "MM+ROLZX", "ROLZX+BWT+RANK+ZRLT",
                "UTF", "UTF+BWT+RANK+ZRLT", "LZP+UTF+BWT+LZP", "UTF+PACK+RLT", "UTF+ROLZX",
                "EXE", "EXE+ROLZX", "EXE+PACK+ZRLT", "EXE+BWT+RANK+ZRLT", "MM+EXE", "TEXT", "TEXT+UTF+BWT+RANK+ZRLT", "TEXT+PACK",
                "TEXT+ROLZX", "LZP+TEXT", "EXE+TEXT", "DNA", "DNA+RLT"]
NEWER_ENTS = ["RANGE", "CM", "TPAQ", "TPAQX"]
NEWER_KINDS = ["walk", "alpha12", "acgt", "repeats", "utf8", "x86"]
BINARY_ENTS = ("CM", "TPAQ", "TPAQX")
CM_MAX = 65536
FPAQ_MAX = 300000


def gen(kind, n, rng):
    if kind == "text": return vectors.make(("text", n, int(rng.integers(1, 1000))))
    if kind == "mixed": return vectors.make(("mixed", n, int(rng.integers(1, 1000))))
    if kind == "rand": return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "runs":
        out = bytearray()
        while len(out) < n:
            out += bytes([int(rng.integers(0, 256))]) * int(rng.geometric(0.02 if rng.random() < 0.3 else 0.4))
        return bytes(out[:n])
    if kind == "sparse":
        a = np.zeros(n, dtype=np.uint8); k = max(1, n // 50)
        a[rng.integers(0, n, k)] = rng.integers(1, 256, k, dtype=np.uint8)
        return a.tobytes()
    if kind == "walk":
        # steps of -3 .. 3 reflected into 40 .. 215: the deltas stay small and the value never wraps
        steps = rng.integers(-3, 4, n)
        w = np.abs((128 + np.cumsum(steps) - 40) % 350)
        return (40 + np.where(w > 175, 350 - w, w)).astype(np.uint8).tobytes()
    if kind == "alpha12":
        p = np.arange(12, 0, -1, dtype=np.float64)
        return np.frombuffer(b"etaoinshrdl ", dtype=np.uint8)[rng.choice(12, size=n, p=p / p.sum())].tobytes()
    if kind == "acgt":
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    if kind == "repeats":
        return knzlib.corpus().repeats(n, int(rng.integers(1, 1000)))
    if kind == "utf8":
        return utf_cases.utf8(n, int(rng.integers(1, 1000)))
    if kind == "x86":
        return bytes(exe_cases.x86(n, int(rng.integers(1, 1000))))
    return bytes((rng.integers(0, 3, n, dtype=np.uint8) * 37 + 65).astype(np.uint8))


def draw(rng, chains, ents, kinds):
    """One case: (chain, coder, block size, length, kind, jobs, checksum)."""
    chain = chains[int(rng.integers(0, len(chains)))]
    ent = ents[int(rng.integers(0, len(ents)))]
    bs = int(rng.choice([1024, 4096, 65536, 262144, 1 << 20])) if ent not in ("FPAQ",) + BINARY_ENTS and "SRT" not in chain else int(rng.choice([1024, 4096, 65536]))
    n = int(rng.integers(0, 6 * bs + 7)) if bs <= 65536 else int(rng.integers(bs // 2, 3 * bs))
    if ent == "FPAQ": n = min(n, FPAQ_MAX)
    if ent in BINARY_ENTS: n = min(n, CM_MAX)
    kind = kinds[int(rng.integers(0, len(kinds)))]
    jobs = int(rng.choice([1, 2, 3, 8]))
    ck = int(rng.choice([0, 0, 32, 64]))
    return chain, ent, bs, n, kind, jobs, ck


def is_newer(chain, ent):
    return chain in NEWER_CHAINS or ent in NEWER_ENTS


class Expected:
    """The expected stream of a case, and the verdict on a stream that does not decode: from the oracle where it knows the chain and
    the coder, from the reference build otherwise."""

    def __init__(self, O, R, newer):
        self.lib = R if newer else O
        self.newer = newer

    def stream(self, d, chain, ent, bs, jobs, ck):
        return self.lib.compress(d, chain, ent, bs, headerless=1, jobs=jobs, checksum=ck)

    def cannot_read_its_own(self, d, chain, ent, bs, jobs, ck):
        rc1, full = self.lib.compress(d, chain, ent, bs, headerless=0, jobs=jobs, checksum=ck, orig_size=len(d))
        rc2, back = self.lib.decompress(full, len(d) + bs)
        return rc1 == 0 and (rc2 != 0 or back != d)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    budget = float(sys.argv[2]) if len(sys.argv) > 2 else 60.0
    mode = sys.argv[3] if len(sys.argv) > 3 else "first"
    if mode not in ("first", "newer"):
        sys.exit("usage: gpu_soak.py SEED SECONDS [first|newer]")
    knzlib.load_pkg()
    hipapi = importlib.import_module("kanzi_amd.hipapi")
    O = knzlib.Oracle()
    R = knzlib.Ref() if mode == "newer" and os.path.exists(knzlib.REF_SO) else None        # (only what build() left in oracle/_ref)
    ctx = hipapi.Context(0)
    rng = np.random.default_rng(seed)
    chains, ents, kinds = (CHAINS, ENTS, KINDS) if mode == "first" else (CHAINS + NEWER_CHAINS, ENTS + NEWER_ENTS, KINDS + NEWER_KINDS)
    t0 = time.time(); n_ok = [0, 0]; bad = 0; n_refbug = 0; n_skipped = 0; per_chain = {}
    while time.time() - t0 < budget:
        chain, ent, bs, n, kind, jobs, ck = draw(rng, chains, ents, kinds)
        d = gen(kind, n, rng) if n else b""
        # expanding first stages on incompressible input trip the reference's own out-of-bounds writes: skip them
        if chain.split("+")[0] in ("ZRLT", "RLT", "SRT") and kind in ("rand",): continue
        newer = is_newer(chain, ent)
        if newer and R is None:
            n_skipped += 1
            continue
        exp = Expected(O, R, newer)
        rc, ref = exp.stream(d, chain, ent, bs, jobs, ck)
        p = ctx.params(chain, ent, bs, ck, jobs=jobs)
        cap = ctx.encode_bound(p, len(d)) + 64
        if ent in BINARY_ENTS: cap += 32 * len(d)            # knz_hip_encode_bound is these coders' first tier (include/knz_hip.h)
        d_in = ctx.malloc(len(d) + 64); d_out = ctx.malloc(cap)
        ctx.h2d(d_in, d)
        ok = dok = False
        refbug = False
        try:
            bits = ctx.encode_blocks(p, d_in, len(d), d_out, cap, finish=1)
            got = ctx.d2h(d_out, (bits + 7) // 8)
            ok = got == ref
        except Exception as ex:
            print("EXC encode", ex)
        d_enc = ctx.malloc(len(ref) + 64); d_dec = ctx.malloc(len(d) + 2 * bs + 64); ctx.h2d(d_enc, ref)
        try:
            ob, eb, nb = ctx.decode_blocks(p, d_enc, 8 * len(ref), 0, d_dec, len(d) + bs)
            dok = ctx.d2h(d_dec, ob) == d if ob else (len(d) == 0)
        except Exception as ex:
            # some streams the reference emits cannot be decoded by the reference either (reference bugs):
            # refusing them is the bit-exact behaviour
            refbug = exp.cannot_read_its_own(d, chain, ent, bs, jobs, ck)
            dok = refbug
            if not refbug: print("EXC decode", ex)
        ctx.free(d_enc); ctx.free(d_dec)
        ctx.free(d_in); ctx.free(d_out)
        if ok and dok:
            n_ok[int(newer)] += 1
            n_refbug += int(refbug)
            if chain in NEWER_CHAINS: per_chain[chain] = per_chain.get(chain, 0) + 1
        else:
            bad += 1
            print("MISMATCH chain=%s ent=%s bs=%d n=%d kind=%s jobs=%d ck=%d enc=%s dec=%s" % (chain, ent, bs, n, kind, jobs, ck, ok, dok), flush=True)
            open("/tmp/soak_fail_%d.bin" % bad, "wb").write(d)
    if mode == "newer":
        print("cases ok per newer chain:", ", ".join("%s %d" % (c, per_chain[c]) for c in NEWER_CHAINS if c in per_chain))
    print("soak seed", seed, "cases ok", sum(n_ok), "(first generation %d, newer stages %d; of which undecodable by the reference too: %d; skipped for want of the reference build: %d)"
          % (n_ok[0], n_ok[1], n_refbug, n_skipped), "bad", bad, "%.0f s" % (time.time() - t0))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
