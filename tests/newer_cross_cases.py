"""Input, chains and damage of the cross-cutting tests of the newer stages (tests/test_gpu_newer_cross.py): tests/golden/newer_cross.json
stores what the reference computed from them (tools/make_newer_cross_golden.py), the tests rebuild the bytes."""
import numpy as np

import knzlib
import mm_cases
import pack_cases

BS = 16384
N = 17 * BS + 1234

# (chain, coder, checksum, jobs)
CHAINS = [("LZP+BWTS+RANK+ZRLT", "RANGE", 32, 1), ("PACK+MM", "CM", 0, 1), ("PACK+BWT+MTFT+ZRLT", "RANGE", 64, 3),
          ("MM+LZP+BWT+SRT+ZRLT", "HUFFMAN", 0, 2)]
VARIANTS = 6


def make_input():
    """17 blocks of 16 KiB and a tail of 1,234 bytes: text with copied spans (LZP, PACK), an ACGT stretch (PACK's 2-bit mode), a random
    walk (MM) and random bytes (every stage refuses; CM and RANGE expand). The stretches do not end on block boundaries."""
    parts = [knzlib.corpus().repeats(5 * BS + 777, 71), pack_cases.alphabet(4 * BS - 300, 4, 72), mm_cases.walk(4 * BS + 100, 73, 1, 0.0)]
    rest = N - sum(len(p) for p in parts)
    parts.append(np.random.default_rng(74).integers(0, 256, rest, dtype=np.uint8).tobytes())
    d = b"".join(parts)
    assert len(d) == N
    return d


def damage(stream, first, chain_idx, variant):
    """A damaged copy of `stream`, whose bytes below `first` (the stream header) stay: byte flips, a 64-byte overwritten range or a cut,
    the kinds of tests/test_gpu_parity.py::test_corrupted_streams_fail_cleanly."""
    rng = np.random.default_rng(1000 * chain_idx + variant)
    buf = bytearray(stream)
    if variant % 3 == 0:
        for _ in range(1 + variant):
            buf[int(rng.integers(first, len(buf)))] ^= int(rng.integers(1, 256))
    elif variant % 3 == 1:
        a = int(rng.integers(first, len(buf) - 64))
        buf[a:a + 64] = bytes(rng.integers(0, 256, 64, dtype=np.uint8))
    else:
        buf = buf[:int(rng.integers(first + 8, len(buf)))]
    return bytes(buf)
