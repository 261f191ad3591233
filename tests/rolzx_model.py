"""ROLZX (ROLZCodec2, transform id 12) restated in plain Python from its description: a ring of 32 positions per 16-bit key, a greedy
parse, and an adaptive binary range coder of its own over 56 bits that moves 32 bits at a time. Covers the data type (EXE: keys 3 bytes
back; DNA: hashed 8-byte keys and matches of 7 and more), the chunks of 16 MiB (`chunk` shrinks them for tests of the model itself) and
the two places where the device refuses what the reference does by writing outside its buffers. Both functions count the paths an
input takes. tests/test_rolzx_model.py pins this file to the reference. Test infrastructure only: byte loops, slow on purpose."""
import collections

CHUNK = 1 << 24
HASH = 200002979
HASH_MASK = 0xFF000000
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
TOP = 0x00FFFFFFFFFFFFFF
MAX_MATCH = 258
MIN_BLOCK = 64
MAX_BLOCK = 1 << 30
UNDEFINED, EXE, DNA = 0, 3, 6


def max_encoded(n):
    """ROLZCodec2::getMaxEncodedLength"""
    return n + (1024 if n < 32768 else n >> 5)


def simple_type(data):
    """Global::detectSimpleType on the histogram of the whole block"""
    f = collections.Counter(data)
    n = len(data)
    if sum(f[c] for c in b"acgntuACGNTU") > n - n // 12:
        return DNA
    if sum(f[c] for c in b"0123456789+-*/=,.:; ") == n:
        return 4
    b64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
    if (1 if f[0x3D] == 1 else 0) + sum(f[c] for c in b64) == n:
        return 5
    if len(f) == 256:
        return 7
    return 9 if len(f) <= 4 else UNDEFINED


def key_of(buf, p, delta):
    """getKey1 / getKey2 of the bytes at p - delta"""
    if delta == 8:
        return (((int.from_bytes(buf[p - 8:p], "little") * HASH) & M64) >> 40) & 0xFFFF
    return buf[p - delta] | (buf[p - delta + 1] << 8)


def hash32(buf, p):
    return (((int.from_bytes(buf[p:p + 4], "little") << 8) & M32) * HASH) & HASH_MASK


class Encoder:
    def __init__(self, out):
        self.low, self.high, self.out = 0, TOP, out
        self.reset()

    def reset(self):
        self.lit = [0x7FFF] * (256 << 9)
        self.idx = [0x7FFF] * (256 << 5)

    def encode(self, probs, ctx, val, n):
        c1 = 1
        for i in range(n - 1, -1, -1):
            bit = (val >> i) & 1
            p = probs[ctx + c1]
            split = (((self.high - self.low) >> 4) * (p >> 4)) >> 8
            if bit:
                self.high = self.low + split
                probs[ctx + c1] = p - ((p - 0xFFFF + 32) >> 5)
            else:
                self.low += split + 1
                probs[ctx + c1] = p - (p >> 5)
            c1 += c1 + bit
            while ((self.low ^ self.high) >> 24) == 0:
                self.out += ((self.high >> 32) & M32).to_bytes(4, "big")
                self.low = (self.low << 32) & M64
                self.high = ((self.high << 32) | M32) & M64

    def dispose(self):
        self.out += self.low.to_bytes(8, "big")


class Decoder:
    def __init__(self, buf, idx):
        self.buf, self.pos = buf, idx + 8
        self.low, self.high, self.cur = 0, TOP, int.from_bytes(buf[idx:idx + 8], "big")
        self.short = False                   # it would have read 4 bytes that do not lie inside the input
        self.reset()

    def reset(self):
        self.lit = [0x7FFF] * (256 << 9)
        self.idx = [0x7FFF] * (256 << 5)

    def decode(self, probs, ctx, n):
        c1 = 1
        for _ in range(n):
            p = probs[ctx + c1]
            mid = self.low + ((((self.high - self.low) >> 4) * (p >> 4)) >> 8)
            if mid >= self.cur:
                self.high = mid
                probs[ctx + c1] = p - ((p - 0xFFFF + 32) >> 5)
                c1 += c1 + 1
            else:
                self.low = mid + 1
                probs[ctx + c1] = p - (p >> 5)
                c1 += c1
            while ((self.low ^ self.high) >> 24) == 0:
                if self.pos + 4 > len(self.buf):
                    self.short = True
                    return 0
                self.low = (self.low << 32) & TOP
                self.high = ((self.high << 32) | M32) & TOP
                self.cur = ((self.cur << 32) | int.from_bytes(self.buf[self.pos:self.pos + 4], "big")) & TOP
                self.pos += 4
        return c1 & ((1 << n) - 1)


def _length(buf, a, b, max_match):
    """A candidate's length as findMatch steps it: whole 8-byte words while n < maxMatch, so it may overshoot maxMatch by up to 7."""
    n = 0
    while n < max_match:
        if buf[a + n:a + n + 8] != buf[b + n:b + n + 8]:
            while buf[a + n] == buf[b + n]:
                n += 1
            break
        n += 8
    return n


def _find_match(buf, base, pos, end, key, matches, counters, min_match, paths):
    counter = counters[key]
    row = key << 5
    h = hash32(buf, base + pos)
    best_len, best_idx = 0, -1
    max_match = min(MAX_MATCH, end - pos) - 8
    if max_match <= 0:
        paths["no_room_for_a_match"] += 1
    for i in range(counter, counter - 32, -1):
        ref = matches[row + (i & 31)]
        if (ref & HASH_MASK) != h:
            continue
        if ref == 0:
            paths["zero_entry_is_a_candidate"] += 1
        ref &= 0xFFFFFF
        if buf[base + ref + best_len] != buf[base + pos + best_len]:
            continue
        n = _length(buf, base + ref, base + pos, max_match)
        if n > max_match > 0:
            paths["length_overshoots"] += 1
        if n == best_len and n > 0:
            paths["equal_length_newer_stays"] += 1
        if n > best_len:
            best_idx, best_len = counter - i, n
            if best_len == max_match:
                paths["scan_ends_at_exact_length"] += 1
                for k in range(i - 1, counter - 32, -1):          # (diagnosis only: what the scan no longer sees)
                    r2 = matches[row + (k & 31)]
                    if (r2 & HASH_MASK) == h and _length(buf, base + (r2 & 0xFFFFFF), base + pos, max_match) > best_len:
                        paths["longer_candidate_behind_exact"] += 1
                break
    if counter == 31:
        paths["counter_wraps"] += 1
    counters[key] = (counter + 1) & 31
    matches[row + counters[key]] = h | pos
    if 0 < best_len < min_match:
        paths["below_min_match_%d" % best_len] += 1
    if best_len < min_match:
        return -1
    if best_len == min_match:
        paths["match_of_min_match"] += 1
    if best_len >= 250:
        paths["match_of_maximum"] += 1
    if best_idx:
        paths["match_index_nonzero"] += 1
    return (best_idx << 16) | (best_len - min_match)


def forward(src, cap, dtype=UNDEFINED, chunk=CHUNK):
    """(ok, output, data type afterwards, paths). The device's verdict: it refuses as soon as the bytes written reach the input's length,
    which is where the reference's final check fails too."""
    paths = collections.Counter()
    count = len(src)
    if count == 0:
        return True, b"", dtype, paths
    if count < MIN_BLOCK or count > MAX_BLOCK or cap < max_encoded(count):
        paths["refuse_early"] += 1
        return False, b"", dtype, paths
    if dtype == UNDEFINED:
        dtype = simple_type(src)
    delta, min_match, flags = 2, 3, 0
    if dtype == EXE:
        delta, flags = 3, 8
        paths["exe"] += 1
    elif dtype == DNA:
        delta, min_match, flags = 8, 7, 4
        paths["dna"] += 1
    out = bytearray(count.to_bytes(4, "big") + bytes([flags]))
    re = Encoder(out)
    counters = [0] * 65536
    src_end = count - 4
    size_chunk = min(count, chunk)
    start = 0
    base, i = 0, 0
    while start < src_end:
        matches = [0] * (65536 << 5)
        end_chunk = min(start + size_chunk, src_end)
        size_chunk = end_chunk - start
        re.reset()
        base, i = start, 0
        if start:
            paths["second_chunk"] += 1
        for _ in range(min(src_end - start, 8)):
            re.encode(re.lit, 0, 0x100 | src[base + i], 9)
            i += 1
        while i < size_chunk:
            if len(out) >= count:
                paths["refuse_output_reaches_count"] += 1
                return False, b"", dtype, paths
            ctx = src[base + i - 1]
            m = _find_match(src, base, i, size_chunk, key_of(src, base + i, delta), matches, counters, min_match, paths)
            if m < 0:
                re.encode(re.lit, ctx << 9, 0x100 | src[base + i], 9)
                i += 1
                continue
            re.encode(re.lit, ctx << 9, m & 0xFFFF, 9)
            re.encode(re.idx, ctx << 5, m >> 16, 5)
            i += (m & 0xFFFF) + min_match
        start = end_chunk
    for _ in range(4):
        re.encode(re.lit, src[base + i - 1] << 9, 0x100 | src[base + i], 9)
        i += 1
    re.dispose()
    if len(out) >= count:
        paths["refuse_output_reaches_count"] += 1
        return False, b"", dtype, paths
    return True, bytes(out), dtype, paths


def inverse(src, cap, chunk=CHUNK):
    """(ok, output, paths). Statement by statement ROLZCodec2::inverse, with the device's two refusals where the reference goes outside its
    buffers: `refuse_short_read` (4 bytes that do not lie inside the input; the reference ends with srcIdx != count) and
    `refuse_write_outside` (a literal or a copy that would end behind the decoded length; the reference writes there)."""
    paths = collections.Counter()
    count = len(src)
    if count == 0:
        return True, b"", paths
    if count < 5 or count > MAX_BLOCK:
        paths["refuse_early"] += 1
        return False, b"", paths
    dst_end = int.from_bytes(src[:4], "big")
    if dst_end >= 1 << 31:
        dst_end -= 1 << 32
    if dst_end <= 0 or dst_end > cap:
        paths["refuse_length_field"] += 1
        return False, b"", paths
    if count < 13:
        paths["refuse_short_read"] += 1
        return False, b"", paths
    delta, min_match = 2, 3
    if (src[4] & 0x0E) == 8:
        delta = 3
    elif (src[4] & 0x0E) == 4:
        delta, min_match = 8, 7
    rd = Decoder(src, 5)
    counters = [0] * 65536
    dst = bytearray(dst_end)
    size_chunk = min(dst_end, chunk)
    start, out = 0, 0

    def fail(why):
        paths[why] += 1
        return False, b"", paths

    while start < dst_end:
        matches = [0] * (65536 << 5)
        end_chunk = min(start + size_chunk, dst_end)
        size_chunk = end_chunk - start
        rd.reset()
        base, i = out, 0
        if start:
            paths["second_chunk"] += 1
        for _ in range(min(dst_end - out, 8)):
            val = rd.decode(rd.lit, 0, 9)
            if rd.short:
                return fail("refuse_short_read")
            if (val >> 8) == 0:
                return fail("refuse_match_among_first_literals")
            dst[base + i] = val & 0xFF
            i += 1
        while i < size_chunk:
            if base + i >= dst_end:
                return fail("refuse_write_outside")
            saved = i
            key = key_of(dst, base + i, delta)
            row = key << 5
            ctx = dst[base + i - 1]
            val = rd.decode(rd.lit, ctx << 9, 9)
            if rd.short:
                return fail("refuse_short_read")
            if val >> 8:
                dst[base + i] = val & 0xFF
                i += 1
                paths["literal"] += 1
            else:
                match_len = val & 0xFF
                if i + match_len + 3 > dst_end:
                    return fail("refuse_sanity_check")
                if base + i + match_len + min_match > dst_end:
                    return fail("refuse_write_outside")
                match_idx = rd.decode(rd.idx, ctx << 5, 5)
                if rd.short:
                    return fail("refuse_short_read")
                ref = matches[row + ((counters[key] - match_idx) & 31)]
                n = match_len + min_match
                if i - ref < n:
                    paths["copy_overlaps"] += 1
                for k in range(n):
                    dst[base + i + k] = dst[base + ref + k]
                i += n
                paths["match"] += 1
            counters[key] = (counters[key] + 1) & 255
            matches[row + (counters[key] & 31)] = saved
        start = end_chunk
        out += i
    if rd.pos != count:
        return fail("refuse_input_not_used_up")
    return True, bytes(dst[:out]), paths
