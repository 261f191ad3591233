"""The header helpers of kanzi-cpp_amd/csrc/ent_header.hpp on their own, on the fiber emulation (tests/emu/ent_header_emu.cpp, built
with AddressSanitizer like the other stand-alone emulator programs): the alphabet writer against range_model.put_alphabet (pinned to
the reference by test_range_model.py) and against the alphabet reader through both of its fetchers, the var-int reader in both of its
forms, and the scans' LDS header window against bits taken from the byte array here. The kernels that use the helpers are covered
by test_emu_kernels.py, test_emu_entropy_edges.py and their GPU counterparts."""
import random
import struct
import subprocess

import pytest

import range_model as rm
from test_emu_kernels import build

WIN_BITS = 8192


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build("ent_header_emu", tmp_path_factory.mktemp("ent_header"), extra=["-fsanitize=address", "-g", "-fno-omit-frame-pointer"])


def run(exe, tmp_path, cases):
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)) + b"".join(cases))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    return lines


def alphabets():
    rng = random.Random(20260)
    sets = [[], [0], [7], [8], [255], list(range(256)), [s for s in range(256) if s != 100], list(range(255)), list(range(1, 256))]
    for last in range(32):
        # the highest symbol in mask byte `last`, anything below it
        s = set(rng.sample(range(8 * last + 8), rng.randint(0, min(8 * last + 7, 40))))
        s.add(8 * last + rng.randrange(8))
        sets.append(sorted(s))
    return sets


def test_alphabet_written_and_read_back(exe, tmp_path):
    sets = alphabets()
    assert sorted({a[-1] >> 3 for a in sets if 0 < len(a) < 256}) == list(range(32))       # every lastMask
    jobs = [(a, pos0) for a in sets for pos0 in (0, 13)]
    cases = []
    for a, pos0 in jobs:
        mask = bytearray(32)
        for s in a:
            mask[s >> 3] |= 1 << (s & 7)
        cases.append(struct.pack("<II", 1, pos0) + bytes(mask))
    for (a, pos0), line in zip(jobs, run(exe, tmp_path, cases)):
        t = line.split()
        bw = rm.BitWriter()
        bw.put(0, pos0)
        rm.put_alphabet(bw, a)
        bits = bw.n - pos0
        assert t[0] == "A" and int(t[1]) == bits, (a, pos0, line)
        assert bytes.fromhex(t[2]) == bw.bytes(), (a, pos0, line)
        present = "".join("%x" % sum(1 << k for k in range(4) if 4 * lane + k in a) for lane in range(64))
        ranks = ",".join(str(sum(1 for s in a if s < 4 * lane)) for lane in range(64))
        for k in (3, 8):                                                            # the LDS window, then peek_bits
            asz, first, nxt, pres, rk = int(t[k]), int(t[k + 1]), int(t[k + 2]), t[k + 3], t[k + 4]
            assert asz == len(a) and first == (a[0] if a else 0), (a, pos0, line)
            assert nxt == pos0 + bits, (a, pos0, line)                              # advanced by exactly the bits written
            assert pres == present and rk == ranks, (a, pos0, line)


def varint_bytes(v):
    out = bytearray()
    while v >= 128:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def test_varint_forms_agree(exe, tmp_path):
    values = [0, 127, 128, (1 << 14) - 1, 1 << 14, 1 << 21, (1 << 28) - 1, 1 << 28, (1 << 32) - 1]
    bad = [b"\xff\xff\xff\xff\x81", b"\xff\xff\xff\xff\x71", b"\x80\x80\x80\x80\x10"]      # a fifth byte that continues / has bits 4-6
    jobs = [(varint_bytes(v), v, off) for v in values for off in (0, 3)] + [(b, None, off) for b in bad for off in (0, 3)]
    cases = []
    for data, v, off in jobs:
        bw = rm.BitWriter()
        bw.put(0, off)
        for byte in data + b"\xa5\x5a":                                             # something behind it that is not part of it
            bw.put(byte, 8)
        raw = bw.bytes()
        cases.append(struct.pack("<III", 2, off, len(raw)) + raw)
    for (data, v, off), line in zip(jobs, run(exe, tmp_path, cases)):
        t = line.split()
        win, src = [int(x) for x in t[1:4]], [int(x) for x in t[4:7]]
        assert t[0] == "V" and win == src, (data, off, line)                          # same value, same advance, same error
        assert win[1] == 8 * len(data), (data, off, line)
        if v is None:
            assert win[2] == 1, (data, off, line)
        else:
            assert win[0] == v and win[2] == 0, (data, off, line)


def bits_of(data, pos, n):
    return (int.from_bytes(data, "big") >> (8 * len(data) - pos - n)) & ((1 << n) - 1)


def test_header_window(exe, tmp_path):
    rng = random.Random(355)
    data = bytes(rng.randrange(256) for _ in range(3075))                              # 3 KiB and three bytes: the last word is partial
    assert len(data) % 4
    READ, PREFETCH = 0, 1
    jobs = []
    for k, n in enumerate((1, 7, 8, 31, 32)):
        base = 1024 + 32 * k
        last = base + WIN_BITS - n
        # (pos, n, need, expected window origin): the window's first bit, its last `need` bits, one bit further -- a reload
        jobs.append([(READ, base, n, n, base), (READ, last, n, n, base), (READ, last + 1, n, n, (last + 1) & ~31)])
        assert (last + 1) & ~31 != base
    end = 8 * (len(data) - 1)
    jobs.append([(READ, 0, 8, 8, 0),
                 (PREFETCH, 12288, 0, 0, None), (READ, 12388, 32, 64, 12288),         # the prefetched window covers it: taken
                 (PREFETCH, 2048, 0, 0, None), (READ, 21000, 8, 8, 21000 & ~31),      # it does not: an exact load, the guess is dropped
                 (READ, 2100, 7, 7, 2100 & ~31),                                      # (... dropped: not 2048)
                 (READ, 12388, 1, 40, 12388 & ~31),
                 (READ, end, 8, 8, end & ~31)])                                       # the last whole byte of the stream
    cases = [struct.pack("<II", 3, len(data)) + data + struct.pack("<I", len(ops)) + b"".join(struct.pack("<IIII", *op[:4]) for op in ops)
             for ops in jobs]
    for ops, line in zip(jobs, run(exe, tmp_path, cases)):
        reads = [op for op in ops if op[0] == READ]
        t = line.split()
        assert t[0] == "W" and len(t) == 1 + len(reads), line
        for (_, pos, n, need, origin), got in zip(reads, t[1:]):
            value, at = (int(x) for x in got.split("@"))
            assert value == bits_of(data, pos, n), (pos, n, line)
            assert at == origin, (pos, n, need, line)
