"""A Python restatement of kanzi's CM entropy coder (entropy id 6), written from the format: a context-mixing predictor
(counter1[256][257] at 32768, counter2[512][17] at j << 12 with cell 16 at 65536, the table of bitstream version 6) in front of a
binary arithmetic coder on a 56-bit interval that leaves 32 bits whenever the top 32 agree. A block is coded in chunks of
max(count, 64) bytes, or count >> 3 / count >> 4 from `big` bytes up (64 MiB in the format; a parameter here); a chunk is a var-int
payload byte count, the payload and 56 bits of low | 0xFFFFFF.

Test infrastructure only. test_cm_model.py pins it against the reference's streams recorded in tests/golden/cm.json before any other
test uses it.
"""
from range_model import BitReader, BitWriter

BIG = 1 << 26
TOP = (1 << 56) - 1
MASK24 = (1 << 24) - 1
MASK32 = (1 << 32) - 1


class BadStream(ValueError):
    pass


class Predictor:
    def __init__(self):
        self.c1 = self.c2 = 0
        self.ctx = 1
        self.run = 0
        self.t1 = [[32768] * 257 for _ in range(256)]
        self.t2 = [[j << 12 for j in range(16)] + [65536] for _ in range(512)]

    def get(self):
        r = self.t1[self.ctx]
        p = (13 * (r[256] + r[self.c1]) + 6 * r[self.c2]) >> 5
        self.row, self.idx = self.t2[self.ctx | self.run], p >> 12
        return (p + p + 3 * (self.row[self.idx] + self.row[self.idx + 1]) + 64) >> 7

    def update(self, bit):
        r, q, i = self.t1[self.ctx], self.row, self.idx
        if bit:
            r[256] -= (r[256] - 65536 + 16) >> 2
            r[self.c1] -= (r[self.c1] - 65536 + 16) >> 4
            q[i] -= (q[i] - 65536 + 16) >> 6
            q[i + 1] -= (q[i + 1] - 65536 + 16) >> 6
        else:
            r[256] -= r[256] >> 2
            r[self.c1] -= r[self.c1] >> 4
            q[i] -= q[i] >> 6
            q[i + 1] -= q[i + 1] >> 6
        self.ctx = 2 * self.ctx + bit
        if self.ctx > 255:
            self.c2, self.c1, self.ctx = self.c1, self.ctx & 0xFF, 1
            self.run = 0x100 if self.c1 == self.c2 else 0


def chunk_len(count, big=BIG):
    length = max(count, 64)
    if length >= big:
        length = count >> 3 if length // 8 < big else count >> 4
    return length


def put_varint(bw, v):
    while v >= 128:
        bw.put(0x80 | (v & 0x7F), 8)
        v >>= 7
    bw.put(v, 8)


def get_varint(br):
    v = br.get(8)
    res, shift = v & 0x7F, 7
    while v >= 128:
        v = br.get(8)
        if shift == 28:
            if v >= 128 or v & 0x70:
                raise BadStream("var-int")
            return res | ((v & 0x0F) << shift)
        res |= (v & 0x7F) << shift
        shift += 7
    return res


def encode(data, big=BIG, bw=None, payloads=None, chooser=None):
    """(bytes, bits) of the block's entropy section; payloads (a list) receives the payload byte count of every chunk. With a
    chooser, the bits come from chooser(split) instead of the data (the adversary of cm_cases) and the bytes they spell are returned
    too."""
    own = bw is None
    bw = bw or BitWriter()
    start = bw.n
    pr = Predictor()
    low, high = 0, TOP
    n, length = len(data), chunk_len(len(data), big)
    spelled = bytearray()
    for s in range(0, n, length):
        pay = bytearray()
        for v in data[s:s + length]:
            made = 0
            for k in range(7, -1, -1):
                split = pr.get()
                bit = chooser(split) if chooser else (v >> k) & 1
                made = 2 * made + bit
                mid = low + ((((high - low) >> 4) * split) >> 8)
                if bit:
                    high = mid
                else:
                    low = mid + 1
                pr.update(bit)
                if (low ^ high) >> 24 == 0:
                    pay += ((high >> 24) & MASK32).to_bytes(4, "big")
                    low = (low << 32) & ((1 << 64) - 1)
                    high = ((high << 32) | MASK32) & ((1 << 64) - 1)
            spelled.append(made)
        put_varint(bw, len(pay))
        if pay:
            bw.put(int.from_bytes(pay, "big"), 8 * len(pay))
        bw.put((low | MASK24) & TOP, 56)
        if payloads is not None:
            payloads.append(len(pay))
    if n == 0:
        bw.put(MASK24, 56)
    if chooser:
        return (bw.bytes(), bw.n - start, bytes(spelled)) if own else (bw.n - start, bytes(spelled))
    return (bw.bytes(), bw.n - start) if own else bw.n - start


def adversary(n):
    """n bytes whose every bit is the one the predictor rates less likely (a split of 2048 or more says 1 is likely)."""
    return encode(bytes(n), chooser=lambda split: 0 if split >= 2048 else 1)[2]


def decode(stream, count, start_bit=0, limit=None, big=BIG):
    """(bytes, bits used). BadStream / ValueError where the stream ends early, a var-int exceeds 32 bytes per byte of its chunk, or
    the coder would read behind its payload (the reference reads what its buffer holds there; no stream it writes does that)."""
    br = BitReader(stream, start_bit, limit)
    pr = Predictor()
    low, high = 0, TOP
    out = bytearray()
    length = chunk_len(count, big)
    for s in range(0, count, length):
        size = min(length, count - s)
        sz = get_varint(br)
        if sz > min(size << 5, 0x1FFFFFFF):
            raise BadStream("payload size")
        cur = br.get(56)
        if br.pos + 8 * sz > br.limit:
            raise BadStream("payload past the end")
        pay = br.get(8 * sz).to_bytes(sz, "big") if sz else b""
        index = 0
        for _ in range(size):
            v = 0
            for _ in range(8):
                split = ((((high - low) >> 4) * pr.get()) >> 8) + low
                bit = 1 if split >= cur else 0
                if bit:
                    high = split
                else:
                    low = split + 1
                pr.update(bit)
                v = 2 * v + bit
                if (low ^ high) >> 24 == 0:
                    if index + 4 > sz:
                        raise BadStream("read behind the payload")
                    low = (low << 32) & TOP
                    high = ((high << 32) | MASK32) & TOP
                    cur = ((cur << 32) | int.from_bytes(pay[index:index + 4], "big")) & TOP
                    index += 4
            out.append(v)
    return bytes(out), br.pos - start_bit


# ---- block framing of a stream whose only transform is NONE (what `kanzi -c -t NONE -e CM` writes behind the stream header)
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
