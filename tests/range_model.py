"""A Python restatement of kanzi's RANGE entropy coder (entropy id 4), chunk encoder and decoder, written from the format:
per chunk of 32,768 bytes an alphabet, 3 bits of lr - 8, the frequencies of all symbols but the first in groups of 6 or 8 behind a
4-bit width, then a carry-less range coder over 60-bit low / range that leaves 28 bits at a time.

Test infrastructure only. test_range_model.py pins it against the reference's streams recorded in tests/golden/range.json before any
other test uses it: to build expected bits for the per-stage entry points, to say which branches an input takes (Stats), and to
supply (code - low, range) pairs for the divide test.
"""
CHUNK = 1 << 15
TOP = (1 << 60) - 1
BOTTOM = 0xFFFF
MASK = 0x0FFFFFFF00000000
M64 = (1 << 64) - 1


class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.nacc = 0
        self.n = 0

    def put(self, val, bits):
        self.acc = (self.acc << bits) | (val & ((1 << bits) - 1))
        self.nacc += bits
        self.n += bits
        if self.nacc >= 256:
            keep = self.nacc & 7
            self.buf += (self.acc >> keep).to_bytes(self.nacc >> 3, "big")
            self.acc &= (1 << keep) - 1
            self.nacc = keep

    def bytes(self):
        pad = -self.nacc % 8
        return bytes(self.buf) + (self.acc << pad).to_bytes((self.nacc + pad) // 8, "big")


class BitReader:
    def __init__(self, data, pos=0, limit=None):
        self.data = data
        self.pos = pos
        self.limit = 8 * len(data) if limit is None else limit

    def get(self, bits):
        if self.pos + bits > self.limit:
            raise ValueError("read past the end of the stream")
        a, e = self.pos >> 3, (self.pos + bits + 7) >> 3
        v = int.from_bytes(self.data[a:e], "big")
        self.pos += bits
        return (v >> (8 * e - self.pos)) & ((1 << bits) - 1)


class Stats:
    """What the chunks of one encode did: 28-bit units per coded chunk, times the range was cut back to the next 2^16 border."""

    def __init__(self):
        self.units = []
        self.underflows = 0
        self.second_units = 0       # bytes that left two units
        self.pairs = []             # decoder only: (code - low, range >> lr, lr) per byte when asked for


def log_range(n):
    lr = 12
    while lr > 8 and (1 << lr) > n:
        lr -= 1
    return lr


def normalize(freqs, total, scale):
    """Frequencies scaled to `scale` in place; returns the alphabet."""
    alphabet = [i for i in range(256) if freqs[i]]
    if total == scale or not alphabet:
        return alphabet
    if len(alphabet) == 1:
        freqs[alphabet[0]] = scale
        return alphabet
    s, idx_max = 0, -1
    for i in alphabet:
        sf = freqs[i] * scale
        f = 1 if sf <= total else (sf + (total >> 1)) // total
        freqs[i] = f
        s += f
        if idx_max < 0 or f > freqs[idx_max]:
            idx_max = i
    if s == scale:
        return alphabet
    delta = s - scale
    thr = freqs[idx_max] >> 4
    if abs(delta) <= thr:
        freqs[idx_max] -= delta
        return alphabet
    if delta < 0:
        delta += thr
        freqs[idx_max] += thr
    else:
        delta -= thr
        freqs[idx_max] -= thr
    inc = 1 if delta < 0 else -1
    delta = abs(delta)
    rnd = 0
    while rnd < 5 and delta > 0:
        rnd += 1
        adjusted = 0
        for i in alphabet:
            if freqs[i] <= 2:
                continue
            freqs[i] += inc
            adjusted += 1
            delta -= 1
            if delta == 0:
                break
        if adjusted == 0:
            break
    freqs[idx_max] = max((freqs[idx_max] - delta) & 0xFFFFFFFF, 1)
    return alphabet


def put_alphabet(bw, alphabet):
    if len(alphabet) == 0:
        bw.put(0, 1); bw.put(1, 1)
    elif len(alphabet) == 256:
        bw.put(0, 1); bw.put(0, 1)
    else:
        bw.put(1, 1)
        masks = [0] * 32
        for s in alphabet:
            masks[s >> 3] |= 1 << (s & 7)
        last = alphabet[-1] >> 3
        bw.put(last, 5)
        for m in masks[:last + 1]:
            bw.put(m, 8)


def get_alphabet(br):
    if br.get(1) == 0:
        return list(range(256)) if br.get(1) == 0 else []
    last = br.get(5)
    out = []
    for i in range(last + 1):
        m = br.get(8)
        out += [8 * i + j for j in range(8) if (m >> j) & 1]
    return out


def put_header(bw, alphabet, freqs, lr):
    put_alphabet(bw, alphabet)
    if not alphabet:
        return
    bw.put(lr - 8, 3)
    if len(alphabet) == 1:
        return
    chk = 8 if len(alphabet) >= 64 else 6
    for i in range(1, len(alphabet), chk):
        grp = [freqs[s] - 1 for s in alphabet[i:i + chk]]
        w = max(grp).bit_length()
        bw.put(w, 4)
        if w:
            for g in grp:
                bw.put(g, w)


def encode_chunk(bw, chunk, stats=None):
    n = len(chunk)
    lr = log_range(n)
    freqs = [0] * 256
    for b in chunk:
        freqs[b] += 1
    alphabet = normalize(freqs, n, 1 << lr)
    put_header(bw, alphabet, freqs, lr)
    if len(alphabet) <= 1:
        return
    cum = [0] * 257
    for i in range(256):
        cum[i + 1] = cum[i] + freqs[i]
    low, rng, units = 0, TOP, 0
    for b in chunk:
        rng >>= lr
        low = (low + cum[b] * rng) & M64
        rng = (rng * freqs[b]) & M64
        here = 0
        while True:
            if (low ^ ((low + rng) & M64)) & MASK:
                if rng > BOTTOM:
                    break
                rng = ~(low - 1) & BOTTOM
                if stats:
                    stats.underflows += 1
            bw.put(low >> 32, 28)
            rng = (rng << 28) & M64
            low = (low << 28) & M64
            here += 1
        units += here
        if stats and here > 1:
            stats.second_units += 1
    bw.put(low, 60)
    if stats:
        stats.units.append(units)


def encode(data, stats=None, bw=None):
    """The entropy bits of one block: (bytes, bit count)."""
    own = bw is None
    if own:
        bw = BitWriter()
    n0 = bw.n
    for o in range(0, len(data), CHUNK):
        encode_chunk(bw, data[o:o + CHUNK], stats)
    return (bw.bytes(), bw.n - n0) if own else None


class BadStream(ValueError):
    pass


def decode(stream, count, start_bit=0, limit=None, stats=None):
    """Returns (bytes, bits used). Raises BadStream where the reference throws, ValueError past the end; an empty alphabet ends the
    block at the chunks done so far."""
    br = BitReader(stream, start_bit, limit)
    out = bytearray()
    while len(out) < count:
        n = min(CHUNK, count - len(out))
        alphabet = get_alphabet(br)
        if not alphabet:
            break
        lr = 8 + br.get(3)
        scale = 1 << lr
        if len(alphabet) == 1:
            out += bytes([alphabet[0]]) * n
            continue
        freqs = [0] * 256
        chk = 8 if len(alphabet) >= 64 else 6
        s = 0
        for i in range(1, len(alphabet), chk):
            w = br.get(4)
            if (1 << w) > scale:
                raise BadStream("frequency width")
            for sym in alphabet[i:i + chk]:
                f = br.get(w) + 1 if w else 1
                if f >= scale:
                    raise BadStream("frequency")
                freqs[sym] = f
                s += f
        if scale <= s:
            raise BadStream("frequency sum")
        freqs[alphabet[0]] = scale - s
        cum = [0] * 257
        f2s = []
        for i in range(256):
            cum[i + 1] = cum[i] + freqs[i]
            f2s += [i] * freqs[i]
        low, rng = 0, TOP
        code = br.get(60)
        for _ in range(n):
            rng >>= lr
            if rng == 0:
                raise BadStream("range")
            d = (code - low) & M64
            if stats is not None:
                stats.pairs.append((d, rng, lr))
            c = d // rng
            if c >= scale:
                raise BadStream("cumulative frequency")
            sym = f2s[c]
            low = (low + cum[sym] * rng) & M64
            rng = (rng * freqs[sym]) & M64
            while True:
                if (low ^ ((low + rng) & M64)) & MASK:
                    if rng > BOTTOM:
                        break
                    rng = ~(low - 1) & BOTTOM
                code = ((code << 28) | br.get(28)) & M64
                rng = (rng << 28) & M64
                low = (low << 28) & M64
            out.append(sym)
    return bytes(out), br.pos - start_bit


# ---- block framing of a stream whose only transform is NONE (what `kanzi -c -t NONE -e RANGE` writes behind the stream header)
def put_block(bw, block, checksum_bits=0, checksum=0):
    inner = BitWriter()
    n = len(block)
    ds = 1 if n < 256 else ((n.bit_length() - 1) >> 3) + 1
    copy = n <= 15
    inner.put((0x80 if copy else 0) | (((ds - 1) & 3) << 5) | 0x07, 8)      # NONE applied: skip flags 0x7F
    inner.put(n, 8 * ds)
    if checksum_bits:
        inner.put(checksum, checksum_bits)
    if copy:
        for b in block:
            inner.put(b, 8)
    else:
        encode(block, bw=inner)
    written = inner.n
    lw = 3 if written < 8 else ((written >> 3).bit_length() - 1) + 4
    bw.put(lw - 3, 5)
    bw.put(written, lw)
    bw.put(int.from_bytes(inner.bytes(), "big") >> (-inner.n % 8), inner.n)


def stream(header, header_bits, data, block_size, checksum_bits=0, hasher=None):
    """The whole .knz: header, blocks, end marker."""
    bw = BitWriter()
    bw.put(int.from_bytes(header, "big") >> (8 * len(header) - header_bits), header_bits)
    for o in range(0, len(data), block_size):
        blk = data[o:o + block_size]
        put_block(bw, blk, checksum_bits, hasher(blk) if checksum_bits else 0)
    bw.put(0, 8)
    return bw.bytes()
