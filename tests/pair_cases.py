"""Input and case table of the pair matrix (tests/test_pair_golden.py, tests/test_gpu_pairs.py): every ordered pair of the 14 device
transforms over one input, once in front of NONE and once in front of a rotation of the coders, checksum widths and job counts.
tests/golden/pairs.json stores what the reference computed from them (tools/make_pair_golden.py), the tests rebuild the bytes.
The typed table adds EXE, TEXT and DNA, which read and set the per-block data type: the 93 ordered pairs of the 17 stages that hold one
of the three, over a longer input (tests/golden/pairs_typed.json, same tool)."""
import numpy as np

import exe_cases
import knzlib
import mm_cases
import pack_cases
import utf_cases

BS = 16384
N = 9 * BS + 10

T = ["BWT", "BWTS", "LZ", "LZX", "LZP", "ROLZX", "RLT", "ZRLT", "MTFT", "RANK", "SRT", "PACK", "MM", "UTF"]
E = ["HUFFMAN", "ANS0", "ANS1", "FPAQ", "RANGE", "CM", "TPAQ", "TPAQX"]
PASSES = ("A", "B")

SETS_TYPE = ("PACK", "MM", "UTF", "ROLZX")      # stages that set the per-block data type (api.hip: XfInfo::setsType) ...
IGNORES_TYPE = ("LZ", "LZX")                    # ... and those that would have to read it and do not: refused behind the former
MAY_REFUSE = ("LZ", "LZX", "LZP", "ROLZX", "RLT", "PACK", "MM", "UTF")
BIG_OUTPUT = ("CM", "TPAQ", "TPAQX")            # knz_hip_encode_bound is their first tier (include/knz_hip.h)
MAX_LEFT_OUT = 5                                # per pass, and only chains whose second stage is ZRLT

# The typed table: the three stages that read as well as set the data type, in front of and behind all 17. tests/golden/pairs_typed.json
T_TYPED = T + ["EXE", "TEXT", "DNA"]
N_TYPED = 14 * BS + 10
SETS_TYPE_TYPED = SETS_TYPE + ("EXE", "TEXT", "DNA")
MAY_REFUSE_TYPED = MAY_REFUSE + ("EXE", "TEXT", "DNA")
MAX_LEFT_OUT_TYPED = 0                          # the reference writes, repeats and reads back all 186 cases on this input


def runs(n, seed):
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes([int(rng.integers(0, 256))]) * int(rng.geometric(0.05))
    return bytes(out[:n])


def sparse(n, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=np.uint8)
    k = n // 40
    a[rng.integers(0, n, k)] = rng.integers(1, 256, k, dtype=np.uint8)
    return a.tobytes()


def make_input():
    """Nine blocks of 16 KiB and a tail of 10 bytes (a copy block): text with copied spans, UTF-8, four symbols, a random walk, runs,
    mostly zeros, random bytes, twelve symbols, text. No stretch ends on a block boundary."""
    c = knzlib.corpus()
    parts = [c.repeats(BS + 300, 71), utf_cases.utf8(BS + 500, 5), pack_cases.alphabet(BS - 300, 4, 72),
             mm_cases.walk(BS + 100, 73, 1, 0.0), runs(BS, 3), sparse(BS - 600, 4),
             np.random.default_rng(74).integers(0, 256, BS, dtype=np.uint8).tobytes(), pack_cases.alphabet(BS, 12, 75), c.text(BS + 10, 9)]
    d = b"".join(parts)
    assert len(d) == N
    return d


def make_typed_input():
    """14 blocks of 16 KiB and a tail of 10 bytes: the nine stretches of make_input(), then x86 code, ARM64 code, ACGT, an ELF file
    with two code sections (its header lies 100 bytes into block 12) and text. No stretch ends on a block boundary."""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(81).integers(0, 4, BS - 200)].tobytes()
    parts = [make_input()[:9 * BS], exe_cases.x86(BS + 400, 82), exe_cases.arm(BS - 100, 83), acgt,
             exe_cases.make(["elf", BS, 85, "x86", 0x3E, 64, True, [[1024, 7000, 1], [9000, 6000, 1]]]),
             knzlib.corpus().text(BS - 90, 84)]
    d = b"".join(bytes(p) for p in parts)
    assert len(d) == N_TYPED
    return d


def case(ps, i, j):
    """(chain, coder, checksum, jobs) of the pair T[i] + T[j] in pass `ps`."""
    k = 14 * i + j
    chain = T[i] + "+" + T[j]
    if ps == "A":
        return chain, "NONE", 0, 1
    return chain, E[(i + j) % 8], (0, 32, 64)[k % 3], (1, 2, 3)[(k // 3) % 3]


def case_typed(ps, i, j):
    """(chain, coder, checksum, jobs) of the pair T_TYPED[i] + T_TYPED[j] in pass `ps`: the rule of case() over 17 stages."""
    k = 17 * i + j
    chain = T_TYPED[i] + "+" + T_TYPED[j]
    if ps == "A":
        return chain, "NONE", 0, 1
    return chain, E[(i + j) % 8], (0, 32, 64)[k % 3], (1, 2, 3)[(k // 3) % 3]


def typed_pairs():
    """The 93 ordered pairs (i, j) of T_TYPED with a new stage in either position, in the order of the fixture's rows."""
    return [(i, j) for i in range(17) for j in range(17) if i >= 14 or j >= 14]


def refused_when_encoding(i, j, stages=T, sets_type=SETS_TYPE):
    return stages[i] in sets_type and stages[j] in IGNORES_TYPE


def records(golden, ps):
    """The rows of pass `ps` of tests/golden/pairs.json as dicts by the file's field names; a case left out has `left_out` (the reason)
    in place of what the reference wrote. Checked against the case table row by row."""
    out = []
    for k, row in enumerate(golden["passes"][ps]):
        assert tuple(row[:4]) == case(ps, k // 14, k % 14), (ps, k, row[:4])
        rec = dict(zip(golden["fields"][:4], row[:4]))
        if isinstance(row[4], dict):
            assert len(row) == 5 and list(row[4]) == ["left_out"]
            rec.update(row[4])
        else:
            assert len(row) == len(golden["fields"])
            rec.update(zip(golden["fields"][4:], row[4:]))
        out.append(rec)
    assert len(out) == 14 * 14
    return out


def records_typed(golden, ps):
    """The rows of pass `ps` of tests/golden/pairs_typed.json by (i, j), as records() gives those of pairs.json."""
    rows, pairs = golden["passes"][ps], typed_pairs()
    assert len(rows) == len(pairs) == 93
    out = {}
    for (i, j), row in zip(pairs, rows):
        assert tuple(row[:4]) == case_typed(ps, i, j), (ps, i, j, row[:4])
        rec = dict(zip(golden["fields"][:4], row[:4]))
        if isinstance(row[4], dict):
            assert len(row) == 5 and list(row[4]) == ["left_out"]
            rec.update(row[4])
        else:
            assert len(row) == len(golden["fields"])
            rec.update(zip(golden["fields"][4:], row[4:]))
        out[i, j] = rec
    return out
