"""A Python restatement of kanzi's TPAQ and TPAQX entropy coders (entropy ids 7 and 9), written from the format: the binary arithmetic
coder and chunk framing of CM (tests/cm_model.py) behind the TPAQ predictor of bitstream version 6 -- two small and one big table of
bit-history states, a hash of buffer positions for the match model, mixers of eight weights chosen by the last byte, and one (TPAQ)
or two (TPAQX) logistic adaptive probability maps. The masks of the ring buffer and the hash are size - 1 WITHOUT rounding to a power
of two (version 6), so `-b 10000` gives masks 9999 and 159999.

The table sizes are parameters (params() gives the format's; states_log forces the states table to 2^k bytes as KNZ_TPAQ_STATES_LOG
does in the library).

Test infrastructure only. test_tpaq_model.py pins it against the reference's streams recorded in tests/golden/tpaq.json.
"""
from range_model import BitReader, BitWriter
from cm_model import BadStream, BIG, TOP, MASK24, MASK32, chunk_len, put_varint, get_varint

M32 = 0xFFFFFFFF
HASH = 0x7FEB352D
MAX_LENGTH = 88
BEGIN_LEARN_RATE = 60 << 7
END_LEARN_RATE = 11 << 7

STATE_TRANSITIONS = (
    (1, 3, 143, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30,
     31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 47, 54, 55, 56, 57, 58, 59, 60,
     61, 62, 63, 64, 65, 66, 67, 68, 69, 6, 71, 71, 71, 61, 75, 56, 77, 78, 77, 80, 81, 82, 83, 84, 85, 86, 87, 88, 77, 90,
     91, 92, 80, 94, 95, 96, 97, 98, 99, 90, 101, 94, 103, 101, 102, 104, 107, 104, 105, 108, 111, 112, 113, 114, 115, 116, 92, 118, 94, 103,
     119, 122, 123, 94, 113, 126, 113, 128, 129, 114, 131, 132, 112, 134, 111, 134, 110, 134, 134, 128, 128, 142, 143, 115, 113, 142, 128, 148, 149, 79,
     148, 142, 148, 150, 155, 149, 157, 149, 159, 149, 131, 101, 98, 115, 114, 91, 79, 58, 1, 170, 129, 128, 110, 174, 128, 176, 129, 174, 179, 174,
     176, 141, 157, 179, 185, 157, 187, 188, 168, 151, 191, 192, 188, 187, 172, 175, 170, 152, 185, 170, 176, 170, 203, 148, 185, 203, 185, 192, 209, 188,
     211, 192, 213, 214, 188, 216, 168, 84, 54, 54, 221, 54, 55, 85, 69, 63, 56, 86, 58, 230, 231, 57, 229, 56, 224, 54, 54, 66, 58, 54,
     61, 57, 222, 78, 85, 82, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (2, 163, 169, 163, 165, 89, 245, 217, 245, 245, 233, 244, 227, 74, 221, 221, 218, 226, 243, 218, 238, 242, 74, 238, 241, 240, 239, 224, 225, 221,
     232, 72, 224, 228, 223, 225, 238, 73, 167, 76, 237, 234, 231, 72, 31, 63, 225, 237, 236, 235, 53, 234, 53, 234, 229, 219, 229, 233, 232, 228,
     226, 72, 74, 222, 75, 220, 167, 57, 218, 70, 168, 72, 73, 74, 217, 76, 167, 79, 79, 166, 162, 162, 162, 162, 165, 89, 89, 165, 89, 162,
     93, 93, 93, 161, 100, 93, 93, 93, 93, 93, 161, 102, 120, 104, 105, 106, 108, 106, 109, 110, 160, 134, 108, 108, 126, 117, 117, 121, 119, 120,
     107, 124, 117, 117, 125, 127, 124, 139, 130, 124, 133, 109, 110, 135, 110, 136, 137, 138, 127, 140, 141, 145, 144, 124, 125, 146, 147, 151, 125, 150,
     127, 152, 153, 154, 156, 139, 158, 139, 156, 139, 130, 117, 163, 164, 141, 163, 147, 2, 2, 199, 171, 172, 173, 177, 175, 171, 171, 178, 180, 172,
     181, 182, 183, 184, 186, 178, 189, 181, 181, 190, 193, 182, 182, 194, 195, 196, 197, 198, 169, 200, 201, 202, 204, 180, 205, 206, 207, 208, 210, 194,
     212, 184, 215, 193, 184, 208, 193, 163, 219, 168, 94, 217, 223, 224, 225, 76, 227, 217, 229, 219, 79, 86, 165, 217, 214, 225, 216, 216, 234, 75,
     214, 237, 74, 74, 163, 217, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
)

STATE_MAP = (
    -31, -400, 406, -547, -642, -743, -827, -901, -901, -974, -945, -955, -1060, -1031, -1044, -956,
    -994, -1035, -1147, -1069, -1111, -1145, -1096, -1084, -1171, -1199, -1062, -1498, -1199, -1199, -1328, -1405,
    -1275, -1248, -1167, -1448, -1441, -1199, -1357, -1160, -1437, -1428, -1238, -1343, -1526, -1331, -1443, -2047,
    -2047, -2044, -2047, -2047, -2047, -232, -414, -573, -517, -768, -627, -666, -644, -740, -721, -829,
    -770, -963, -863, -1099, -811, -830, -277, -1036, -286, -218, -42, -411, 141, -1014, -1028, -226,
    -469, -540, -573, -581, -594, -610, -628, -711, -670, -144, -408, -485, -464, -173, -221, -310,
    -335, -375, -324, -413, -99, -179, -105, -150, -63, -9, 56, 83, 119, 144, 198, 118,
    -42, -96, -188, -285, -376, 107, -138, 38, -82, 186, -114, -190, 200, 327, 65, 406,
    108, -95, 308, 171, -18, 343, 135, 398, 415, 464, 514, 494, 508, 519, 92, -123,
    343, 575, 585, 516, -7, -156, 209, 574, 613, 621, 670, 107, 989, 210, 961, 246,
    254, -12, -108, 97, 281, -143, 41, 173, -209, 583, -55, 250, 354, 558, 43, 274,
    14, 488, 545, 84, 528, 519, 587, 634, 663, 95, 700, 94, -184, 730, 742, 162,
    -10, 708, 692, 773, 707, 855, 811, 703, 790, 871, 806, 9, 867, 840, 990, 1023,
    1409, 194, 1397, 183, 1462, 178, -23, 1403, 247, 172, 1, -32, -170, 72, -508, -46,
    -365, -26, -146, 101, -18, -163, -422, -461, -146, -69, -78, -319, -334, -232, -99, 0,
    47, -74, 0, -452, 14, -57, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
)

MATCH_PRED = (
    0, 64, 128, 192, 256, 320, 384, 448, 512, 576, 640, 704, 768, 832, 896, 960,
    1024, 1038, 1053, 1067, 1082, 1096, 1111, 1125, 1139, 1154, 1168, 1183, 1197, 1211, 1226, 1240,
    1255, 1269, 1284, 1298, 1312, 1327, 1341, 1356, 1370, 1385, 1399, 1413, 1428, 1442, 1457, 1471,
    1486, 1500, 1514, 1529, 1543, 1558, 1572, 1586, 1601, 1615, 1630, 1644, 1659, 1673, 1687, 1702,
    1716, 1731, 1745, 1760, 1774, 1788, 1803, 1817, 1832, 1846, 1861, 1875, 1889, 1904, 1918, 1933,
    1947, 1961, 1976, 1990, 2005, 2019, 2034, 2047,
)

INV_EXP = (0, 8, 22, 47, 88, 160, 283, 492, 848, 1451, 2459, 4117, 6766, 10819, 16608, 24127, 32768, 41409, 48928, 54717, 58770, 61419,
           63077, 64085, 64688, 65044, 65253, 65376, 65448, 65489, 65514, 65528, 65536)


def _tables():
    sq = [0] * 4096
    for x in range(1, 4096):
        w, y = x & 127, x >> 7
        sq[x - 1] = (INV_EXP[y] * (128 - w) + INV_EXP[y + 1] * w) >> 11
    sq[4095] = 4095
    st = [0] * 4096
    n = 0
    for x in range(-2047, 2048):
        v = sq[x + 2047]
        while n <= v:
            st[n] = x
            n += 1
        if n >= 4096:
            break
    st[4095] = 2047
    return sq, st


SQUASH, STRETCH = _tables()


def squash(d):
    return 4095 if d >= 2048 else 0 if d <= -2048 else SQUASH[d + 2047]


def s32(v):
    v &= M32
    return v - (1 << 32) if v & 0x80000000 else v


def params(rbsz, absz, extra):
    """(states bytes, mixers, hash entries, buffer bytes, sse0 contexts, sse1 contexts) of a block of `absz` bytes (after the
    transforms) in a stream of block size `rbsz`; extra = 1 for TPAQX. Bitstream version 6: no rounding to powers of two."""
    if rbsz >= 64 << 20:
        states = 1 << 28
    elif rbsz >= 16 << 20:
        states = 1 << 27
    elif rbsz >= 4 << 20:
        states = 1 << 26
    else:
        states = 1 << 24 if rbsz >= 1 << 20 else 1 << 22
    if absz >= 32 << 20:
        mixers = 1 << 16
    elif absz >= 16 << 20:
        mixers = 1 << 15
    elif absz >= 8 << 20:
        mixers = 1 << 14
    elif absz >= 4 << 20:
        mixers = 1 << 13
    else:
        mixers = 1 << 11 if absz >= 1 << 20 else 1 << 8
    buf = min(rbsz, 64 << 20)
    hsz = min(16 << 20, absz * 16 if absz < 1 << 26 else 1 << 30)
    sh = 2 * extra
    return states << sh, mixers << sh, hsz << sh, buf, 256, 65536 if extra else 256


class APM:
    """LogisticAdaptiveProbMap<false, RATE>: 33 cells per context; get() first moves the two cells of the LAST call."""

    def __init__(self, rate):
        self.rate = rate
        self.index = 0
        self.row0 = [(squash((j - 16) * 128) << 4) & 0xFFFF for j in range(33)]
        self.data = {}

    def cell(self, i):
        v = self.data.get(i)
        return self.row0[i % 33] if v is None else v

    def get(self, bit, pr, ctx):
        g = 65528 if bit else 0
        for i in (self.index, self.index + 1):
            c = self.cell(i)
            self.data[i] = (c + ((g - c) >> self.rate) + bit) & 0xFFFF
        pr = STRETCH[pr]
        self.index = ((pr + 2048) >> 7) + 33 * ctx
        w = pr & 127
        a, b = self.cell(self.index), self.cell(self.index + 1)
        return ((a << 7) + (b - a) * w) >> 11


def create_context(ctx_id, cx):
    cx = (cx * 987654323 + ctx_id) & M32
    cx = ((cx << 16) | (cx >> 16)) & M32
    return (cx * 123456791 + ctx_id) & M32


def hash2(x, y):
    h = s32((x * HASH) ^ (y * HASH))
    return ((h >> 1) ^ (h >> 9) ^ (x >> 2) ^ (y >> 3) ^ HASH) & M32


class Predictor:
    def __init__(self, extra, rbsz, absz, states_log=None):
        states, mixers, hsz, buf, _, _ = params(rbsz, absz, extra)
        if states_log is not None:
            states = 1 << states_log
        self.x = extra
        self.states_mask = states - 1
        self.mixers_mask = (mixers - 1) & ~1
        self.hash_mask = hsz - 1
        self.buf_mask = buf - 1
        self.big = bytearray(states)
        self.small0 = bytearray(1 << 16)
        self.small1 = bytearray(1 << 24)
        self.hashes = {}
        self.buffer = bytearray(buf)
        self.mixers = {}                        # index -> [w0..w7, skew, learn rate]
        self.sse0 = APM(6 if extra else 7)
        self.sse1 = APM(7)
        self.pr = 2048
        self.c0, self.c4, self.c8 = 1, 0, 0
        self.pos = 0
        self.bpos = 8
        self.bin_count = 0
        self.match_len = self.match_pos = self.match_val = 0
        self.hash = 0
        self.mixer = self.mixer_at(0)
        self.inputs = [0] * 8
        self.mix_pr = 2048
        # context pointers: (table, index); cp2..cp6 all into `big`
        self.cp = [(self.small0, 0), (self.small1, 0)] + [(self.big, 0)] * 5
        self.ctx = [0] * 7

    def mixer_at(self, i):
        m = self.mixers.get(i)
        if m is None:
            m = self.mixers[i] = [32768] * 8 + [0, BEGIN_LEARN_RATE]
        return m

    def get(self):
        return self.pr

    def find_match(self):
        if self.match_len > 0:
            if self.match_len < MAX_LENGTH:
                self.match_len += 1
            self.match_pos += 1
            return
        self.match_pos = self.hashes.get(self.hash, 0)
        mask, buf, pos, mp = self.buf_mask, self.buffer, self.pos, self.match_pos
        if mp != 0 and ((pos - mp) & M32) <= mask:
            r = self.match_len + 2
            while r + 6 <= MAX_LENGTH:
                p0 = ((pos - r - 7) & M32) & mask
                p1 = ((mp - r - 7) & M32) & mask
                if p0 > mask - 7 or p1 > mask - 7:
                    break
                diff = int.from_bytes(buf[p0:p0 + 8], "big") ^ int.from_bytes(buf[p1:p1 + 8], "big")
                if diff:
                    tz = (diff & -diff).bit_length() - 1
                    r += (tz >> 4) << 1
                    break
                r += 8
            while r <= MAX_LENGTH:
                if buf[((pos - r - 1) & M32) & mask] != buf[((mp - r - 1) & M32) & mask]:
                    break
                if buf[((pos - r) & M32) & mask] != buf[((mp - r) & M32) & mask]:
                    break
                r += 2
            self.match_len = r - 2

    def update(self, bit):
        # mixer: the pair get / update of one bit
        m = self.mixer
        err = (((bit << 12) - self.mix_pr) * m[9]) >> 10
        if err != 0:
            if m[9] > END_LEARN_RATE:
                m[9] -= 1
            m[8] = s32(m[8] + err)
            inp = self.inputs
            for i in range(8):
                m[i] = s32(m[i] + ((inp[i] * err) >> 12))
        self.c0 = 2 * self.c0 + bit
        self.bpos -= 1
        if self.bpos == 0:
            self.buffer[self.pos & self.buf_mask] = self.c0 & 0xFF
            self.pos += 1
            self.c8 = ((self.c8 << 8) | (self.c4 >> 24)) & M32
            self.c4 = ((self.c4 << 8) | (self.c0 & 0xFF)) & M32
            self.hash = (((((self.hash * HASH) & M32) << 4) + self.c4) & M32) & self.hash_mask
            self.c0 = 1
            self.bpos = 8
            self.bin_count += (self.c4 >> 7) & 1
            c4, c8 = self.c4, self.c8
            self.mixer = self.mixer_at((c4 & self.mixers_mask) + (1 if self.match_len != 0 else 0))
            ctx = self.ctx
            ctx[0] = (c4 & 0xFF) << 8
            ctx[1] = (c4 & 0xFFFF) << 8
            ctx[2] = create_context(2, c4 & 0x00FFFFFF)
            ctx[3] = create_context(3, c4)
            if self.bin_count < (self.pos >> 2):
                ctx[4] = create_context(ctx[1], c4 ^ (c8 & 0xFFFF))
                ctx[5] = (c8 & 0xF0F0F000) | ((c4 & 0xF0F0F000) >> 4)
                if self.x:
                    h1 = c4 & 0x4F4FFFFF if (c4 & 0x80808080) == 0 else c4 & 0x80808080
                    h2 = c8 & 0x4F4FFFFF if (c8 & 0x80808080) == 0 else c8 & 0x80808080
                    ctx[6] = hash2((h1 << 2) & M32, h2 >> 2)
            else:
                ctx[4] = create_context((HASH + self.match_len) & M32, c4 ^ (c4 & 0x000FFFFF))
                ctx[5] = (ctx[0] | (c8 << 16)) & M32
                if self.x:
                    ctx[6] = hash2(c4 & 0xFFFF0000, c8 >> 16)
            self.find_match()
            self.match_val = self.buffer[self.match_pos & self.buf_mask] | 0x100
            self.hashes[self.hash] = self.pos
        c0, ctx, sm, cp = self.c0, self.ctx, self.states_mask, self.cp
        table = STATE_TRANSITIONS[bit]
        for k in range(6):                      # in sequence: two pointers at one address step the state twice
            t, i = cp[k]
            t[i] = table[t[i]]
        cp[0] = (self.small0, ctx[0] + c0)
        cp[1] = (self.small1, ctx[1] + c0)
        cp[2] = (self.big, (ctx[2] + c0) & sm)
        cp[3] = (self.big, (ctx[3] + c0) & sm)
        cp[4] = (self.big, (ctx[4] + c0) & sm)
        cp[5] = (self.big, (ctx[5] ^ c0) & sm)
        p = [STATE_MAP[t[i]] for t, i in cp[:6]]
        p7 = 0
        if self.match_len != 0:
            if c0 == self.match_val >> self.bpos:
                v = MATCH_PRED[self.match_len - 1]
                p7 = v if (self.match_val >> (self.bpos - 1)) & 1 else -v
            else:
                self.match_len = 0
        if self.x:
            # (the state behind the old seventh pointer moves AFTER the six new states were read, TPAQPredictor.hpp:522)
            t, i = cp[6]
            t[i] = table[t[i]]
            cp[6] = (self.big, (ctx[6] + c0) & sm)
            p6 = STATE_MAP[self.big[cp[6][1]]]
        else:
            p6 = p7
        inp = self.inputs = p + [p6, p7]
        m = self.mixer
        dot = s32(sum(a * b for a, b in zip(inp, m)) + m[8] + 65536)
        pr = self.mix_pr = squash(dot >> 17)
        if not self.x:
            if self.bin_count < (self.pos >> 3):
                pr = (3 * self.sse0.get(bit, pr, c0) + pr) >> 2
        else:
            if self.bin_count < (self.pos >> 3):
                pr = self.sse1.get(bit, pr, ctx[0] + c0)
            else:
                if self.bin_count >= (self.pos >> 2):
                    pr = (3 * self.sse0.get(bit, pr, c0) + pr) >> 2
                pr = (3 * self.sse1.get(bit, pr, ctx[0] + c0) + pr) >> 2
        self.pr = pr + (1 if pr < 2048 else 0)


def encode(data, extra, rbsz, big=BIG, bw=None, payloads=None, states_log=None):
    """(bytes, bits) of the block's entropy section; the block's length is the `absz` of the format."""
    own = bw is None
    bw = bw or BitWriter()
    start = bw.n
    pr = Predictor(extra, rbsz, len(data), states_log)
    low, high = 0, TOP
    n, length = len(data), chunk_len(len(data), big)
    for s in range(0, n, length):
        pay = bytearray()
        for v in data[s:s + length]:
            for k in range(7, -1, -1):
                split = pr.pr
                bit = (v >> k) & 1
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
        put_varint(bw, len(pay))
        if pay:
            bw.put(int.from_bytes(pay, "big"), 8 * len(pay))
        bw.put((low | MASK24) & TOP, 56)
        if payloads is not None:
            payloads.append(len(pay))
    if n == 0:
        bw.put(MASK24, 56)
    return (bw.bytes(), bw.n - start) if own else bw.n - start


def decode(stream, count, extra, rbsz, start_bit=0, limit=None, big=BIG, states_log=None):
    """(bytes, bits used). BadStream / ValueError as cm_model.decode."""
    br = BitReader(stream, start_bit, limit)
    pr = Predictor(extra, rbsz, count, states_log)
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
                split = ((((high - low) >> 4) * pr.pr) >> 8) + low
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


# ---- block framing of a stream whose only transform is NONE (what `kanzi -c -t NONE -e TPAQ` writes behind the stream header)
def put_block(bw, block, extra, rbsz, checksum_bits=0, checksum=0):
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
        encode(block, extra, rbsz, bw=inner)
    written = inner.n
    lw = 3 if written < 8 else ((written >> 3).bit_length() - 1) + 4
    bw.put(lw - 3, 5)
    bw.put(written, lw)
    bw.put(int.from_bytes(inner.bytes(), "big") >> (-inner.n % 8), inner.n)


def stream(header, header_bits, data, extra, block_size, checksum_bits=0, hasher=None):
    """The whole .knz: header, blocks, end marker."""
    bw = BitWriter()
    bw.put(int.from_bytes(header, "big") >> (8 * len(header) - header_bits), header_bits)
    for o in range(0, len(data), block_size):
        blk = data[o:o + block_size]
        put_block(bw, blk, extra, block_size, checksum_bits, hasher(blk) if checksum_bits else 0)
    bw.put(0, 8)
    return bw.bytes()
