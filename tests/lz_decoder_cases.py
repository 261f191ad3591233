"""Inputs for the three LZ / LZX decoders of csrc/lz.hip -- k_lz_i_pparse (the parallel parse), k_lz_i_parse (the serial parse that
takes what the parallel one hands on) and k_lz_inverse (one wave per block, knob lz_serial_decode) --, shared by
tests/test_gpu_lz_decoders.py, tests/test_oracle_vs_ref.py and the generator tests/golden/make_first_gen_damage.py.

A block of bitstream version 6 (LZCodec.cpp:470-610) is a 13-byte header -- three little-endian words litEnd (end of the literals = start
of the tokens), nTok (bytes of tokens), nDist (bytes of distances) and a flag byte -- followed by the literals, the tokens, the distances
and the length extensions."""
import struct

import numpy as np

import knzlib

TRANSFORMS = ("LZ", "LZX")
BATCH_BS = 1 << 17
# damaged forms per block, transform and section: fewer in the header's fields, where nearly every change is refused, than in the
# sections behind it, so that the cases test accepting and refusing alike
DRAWS = {"litEnd": 2, "nTok": 2, "nDist": 2, "flags": 2, "literals": 6, "tokens": 6, "extensions": 6}
SEED = 20240

_cache = {}


def blocks():
    """name -> bytes."""
    if _cache:
        return _cache
    c = knzlib.corpus()
    rng = np.random.default_rng(77)
    unit = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    _cache.update({
        "text": c.text(60000, 3),
        "mixed": c.mixed(300000, 2)[250000:290000],
        # literal runs of 7 and more (an extension byte) and of 7 + 255 and more (a long extension)
        "literal_runs": rng.integers(0, 256, 9000, dtype=np.uint8).tobytes() + unit * 2,
        # distances 1, 2, 3, 15, 16, 17: where the reference changes its copy loop, and a match reads what the one before it wrote
        "distances": b"a" * 5000 + b"ab" * 3000 + b"abc" * 2000 + unit[:15] * 300 + unit[:16] * 300 + unit[:17] * 300 + unit * 3,
        # a repeat longer than 65,793 = minimum match + 254 + 65,535, the longest match a token and a three-byte extension hold: the
        # encoder cuts it there and goes on with another match
        "long_match": c.text(3000, 8) + b"q" * 90000 + c.text(3000, 9),
        "tiny": b"xyz" * 10,              # below the codec's smallest block: the forward transform refuses it
    })
    return _cache


def forward_cap(n):
    return n + n // 64 + 18


def batch():
    """The blocks as one buffer of blocks of BATCH_BS bytes: the device decodes a batch whose blocks but the last have one size, so each
    block is filled up with random bytes behind it (literals: the tokens in front of them stay what they are) and the tiny block is the
    short last one."""
    rng = np.random.default_rng(78)
    out = []
    for name, b in blocks().items():
        if name != "tiny":
            out.append(b + rng.integers(0, 256, BATCH_BS - len(b), dtype=np.uint8).tobytes())
    out.append(blocks()["tiny"])
    return b"".join(out)


def parse_v6(enc):
    """[(literals in front, match length, distance)] of a valid block of version 6, by the reference's rules (LZCodec.cpp:518-604)."""
    lit_end, n_tok, n_dist = struct.unpack_from("<III", enc, 0)
    mm = ((enc[12] >> 1) & 7) + 2
    pos = {"s": 13, "t": lit_end, "m": lit_end + n_tok, "l": lit_end + n_tok + n_dist}

    def get_len(k):
        p = pos[k]
        b0 = enc[p]
        if b0 < 254:
            pos[k] += 1
            return b0
        if b0 == 254:
            pos[k] += 3
            return 254 + ((enc[p + 1] << 8) | enc[p + 2])
        pos[k] += 4
        return 255 + ((enc[p + 1] << 16) | (enc[p + 2] << 8) | enc[p + 3])

    out, rep0, rep1 = [], len(enc), len(enc)
    while True:
        token = enc[pos["t"]]
        pos["t"] += 1
        if token & 0x18 == 0:
            mlen = token & 3
            mlen = 3 + mm + get_len("l") if mlen == 3 else mlen + mm
            dist = rep1 if token & 4 else rep0
        else:
            mlen = token & 7
            mlen = 7 + mm + get_len("l") if mlen == 7 else mlen + mm
            dist = 0
            for _ in range((token >> 3) & 3):
                dist = (dist << 8) | enc[pos["m"]]
                pos["m"] += 1
        lit = 0
        if token >= 32:
            lit = 7 + get_len("s") if token >= 0xE0 else token >> 5
            pos["s"] += lit
            if pos["s"] >= lit_end - 13:
                out.append((lit, 0, 0))
                return out
        rep1, rep0 = rep0, dist
        out.append((lit, mlen, dist))


def check(name, enc):
    """The properties the blocks are there for, read from the oracle's encoding."""
    toks = parse_v6(enc)
    if name == "literal_runs":
        assert any(7 <= t[0] < 7 + 254 for t in toks) and any(t[0] >= 7 + 255 for t in toks), name
    if name == "distances":
        assert {1, 2, 3, 15, 16, 17} <= {t[2] for t in toks if t[1] > t[2]}, name       # each with a match that overlaps itself
    if name == "long_match":
        lens = [t[1] for t in toks]
        assert max(lens) == 65793 and lens[lens.index(65793) + 1] > 254, name


def sections(enc):
    """name -> (first byte, bytes) of the places damage goes to. The distances are left alone: a distance damaged to 0 leaves bytes that
    depend on what the destination held before."""
    lit_end, n_tok, n_dist = struct.unpack_from("<III", enc, 0)
    ext = lit_end + n_tok + n_dist
    return {"litEnd": (0, 4), "nTok": (4, 4), "nDist": (8, 4), "flags": (12, 1), "literals": (13, lit_end - 13), "tokens": (lit_end, n_tok),
            "extensions": (ext, len(enc) - ext)}


def damage_cases(name, transform, enc):
    """[(section, damage as (offset, value) pairs)]: DRAWS[section] seeded draws per section of 1 to 3 bytes flipped (one bit) or overwritten, and
    the header cases k_lz_i_pparse hands on by its own checks: no tokens, literals that end inside the header, distances one byte past the
    block."""
    lit_end, n_tok, n_dist = struct.unpack_from("<III", enc, 0)
    rng = np.random.default_rng([SEED, sorted(blocks()).index(name), TRANSFORMS.index(transform)])
    out = []
    for sec, (first, count) in sections(enc).items():
        for _ in range(DRAWS[sec]):
            k = min(int(rng.integers(1, 4)), count)
            offs = sorted(int(x) for x in rng.choice(count, size=k, replace=False)) if count else []
            dmg = []
            for o in offs:
                b = enc[first + o]
                v = b ^ (1 << int(rng.integers(0, 8))) if rng.integers(0, 2) else int(rng.integers(0, 256))
                dmg.append((first + o, v))
            if dmg and (sec, tuple(dmg)) not in out:
                out.append((sec, tuple(dmg)))

    def word(off, value):
        return tuple((off + i, (value >> (8 * i)) & 0xFF) for i in range(4))
    out.append(("nTok=0", word(4, 0)))
    out.append(("litEnd=12", word(0, 12)))
    out.append(("nDist+1", word(8, len(enc) - lit_end - n_tok + 1)))
    return out


def apply(enc, damage):
    b = bytearray(enc)
    for off, v in damage:
        b[off] = v
    return bytes(b)
