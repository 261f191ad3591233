"""LZP (LZPCodec, transform id 14) restated in plain Python from its description: a 16-bit hash of a 4-byte context predicts one
position; matches of 64 bytes and more are replaced by 0xFC, one 0xFE per 254 bytes beyond 64 and the remainder; a literal 0xFC whose
bucket is filled is followed by 0xFF. Both functions also count the paths an input takes (tests/test_lzp_model.py checks that the
fixture takes every one of them). Test infrastructure only: byte loops, slow on purpose."""
import collections

SEED = 0x7FEB352D
MIN_MATCH = 64
MIN_BLOCK = 128
FLAG = 0xFC
M32 = 0xFFFFFFFF


def max_encoded(n):
    return n + 16 if n <= 1024 else n + n // 64


def hash16(ctx):
    return ((SEED * ctx) & M32) >> 16


def le32(b, i):
    return b[i] | (b[i + 1] << 8) | (b[i + 2] << 16) | (b[i + 3] << 24)


def find_match(src, a, b, limit):
    """Whole 8-byte words only: the result may stop up to 7 bytes short of `limit`."""
    n = 0
    while n + 8 <= limit:
        if src[a + n:a + n + 8] != src[b + n:b + n + 8]:
            while src[a + n] == src[b + n]:
                n += 1
            break
        n += 8
    return n


def forward(src, cap):
    """(ok, output, paths)"""
    paths = collections.Counter()
    count = len(src)
    if count == 0:
        return True, b"", paths
    if count < 4 or cap < max_encoded(count) or count < MIN_BLOCK:
        paths["refuse_early"] += 1
        return False, b"", paths
    dst_end = count - (count >> 6)
    table = [0] * 65536
    how = {}                                # position -> (literals since the reload when it was stored, kind of that reload)
    dst = bytearray(src[:4])
    ctx = le32(src, 0)
    s = 4
    run, kind = 0, "start"                  # literals since the last reload (block start or match)
    batch = 4                               # first position of the device's batch of 64 visits
    last_was_match = False
    while s < count - MIN_MATCH and len(dst) < dst_end:
        while s >= batch + 64:
            batch += 64
        h = hash16(ctx)
        ref = table[h]
        table[h] = s
        how[s] = (run, kind)
        best = 0
        if ref != 0 and src[ref + 56:ref + 64] == src[s + 56:s + 64]:
            best = find_match(src, s, ref, count - s)
            if best < MIN_MATCH:
                paths["precheck_passed_match_short"] += 1
        if ref != 0 and ref >= batch:
            paths["same_batch_bucket"] += 1
        if best < MIN_MATCH:
            v = src[s]
            ctx = ((ctx << 8) | v) & M32
            dst.append(v)
            s += 1
            run += 1
            last_was_match = False
            paths["literal"] += 1
            if v == FLAG:
                if ref != 0:
                    paths["fc_escape"] += 1
                    if ref >= batch:
                        paths["fc_escape_same_batch"] += 1
                    if len(dst) >= dst_end:
                        paths["refuse_escape"] += 1
                        return False, b"", paths
                    dst.append(0xFF)
                else:
                    paths["fc_no_escape"] += 1
            continue
        paths["match"] += 1
        if last_was_match:
            paths["match_back_to_back"] += 1
        if run < 4:
            plain = 0
            for k in range(4):
                plain = (plain << 8) | src[s - 4 + k]
            if run in (1, 2, 3) and hash16(plain) != h:
                paths["match_%d_after_%s_mixed_only" % (run, kind)] += 1
        r0, k0 = how[ref]
        if r0 in (1, 2, 3) and k0 == "start":
            plain = 0
            for k in range(4):
                plain = (plain << 8) | src[ref - 4 + k]
            if hash16(plain) != h:
                paths["match_bucket_stored_%d_after_start_mixed_only" % r0] += 1
        if s - ref < best:
            paths["match_overlap_period_%d" % (s - ref)] += 1
        if best == MIN_MATCH:
            paths["match_len_64"] += 1
        if s + best == count:
            paths["match_to_block_end"] += 1
        elif best == (count - s) & ~7:
            paths["match_whole_word_stop"] += 1
        s += best
        ctx = le32(src, s - 4)
        run, kind = 0, "match"
        batch = s
        last_was_match = True
        dst.append(FLAG)
        best -= MIN_MATCH
        paths["fe_run_%s" % (best // 254 if best // 254 < 3 else "3+")] += 1
        if best % 254 == 253:
            paths["len_remainder_253"] += 1
        if best % 254 == 0 and best:
            paths["len_remainder_0"] += 1
        while best >= 254 and len(dst) < dst_end:
            best -= 254
            dst.append(0xFE)
        if len(dst) >= dst_end:
            paths["refuse_fe_run"] += 1
            return False, b"", paths
        dst.append(best)
    while s < count and len(dst) < dst_end:
        while s >= batch + 64:
            batch += 64
        h = hash16(ctx)
        ref = table[h]
        table[h] = s
        paths["tail_literal"] += 1
        if ref != 0 and src[ref:ref + count - s] == src[s:count] and count - s >= 8:
            paths["tail_bucket_predicts_right"] += 1
        v = src[s]
        ctx = ((ctx << 8) | v) & M32
        dst.append(v)
        s += 1
        if v == FLAG:
            if ref != 0:
                paths["fc_escape_tail"] += 1
                if len(dst) >= dst_end:
                    paths["refuse_escape"] += 1
                    return False, b"", paths
                dst.append(0xFF)
            else:
                paths["fc_no_escape_tail"] += 1
    if s == count and len(dst) < dst_end:
        return True, bytes(dst), paths
    paths["refuse_literal"] += 1
    return False, b"", paths


def inverse(src, cap, trace=None):
    """(ok, output, paths); trace, when given, receives (class, input index) of every literal, match flag, 0xFE run and length byte."""
    paths = collections.Counter()
    count = len(src)
    if count == 0:
        return True, b"", paths
    if count < 4 or cap < count:
        paths["refuse_early"] += 1
        return False, b"", paths
    table = [0] * 65536
    dst = bytearray(src[:4])
    ctx = le32(dst, 0)
    s = 4
    while s < count:
        h = hash16(ctx)
        ref = table[h]
        table[h] = len(dst)
        if src[s] != FLAG or ref == 0:
            if len(dst) >= cap:
                paths["refuse_literal"] += 1
                return False, b"", paths
            paths["fc_empty_bucket" if src[s] == FLAG else "literal"] += 1
            if trace is not None:
                trace.append(("literal", s))
            ctx = ((ctx << 8) | src[s]) & M32
            dst.append(src[s])
            s += 1
            continue
        s += 1
        if s >= count:
            paths["refuse_end_after_flag"] += 1
            return False, b"", paths
        if src[s] == 0xFF:
            if len(dst) >= cap:
                paths["refuse_literal"] += 1
                return False, b"", paths
            paths["fc_escaped"] += 1
            ctx = ((ctx << 8) | FLAG) & M32
            dst.append(FLAG)
            s += 1
            continue
        length = MIN_MATCH
        nfe = 0
        if trace is not None:
            trace.append(("flag", s - 1))
            if src[s] == 0xFE:
                trace.append(("fe", s))
        while s < count and src[s] == 0xFE:
            s += 1
            nfe += 1
            length += 254
        if s >= count:
            paths["refuse_end_in_fe_run"] += 1
            return False, b"", paths
        if trace is not None:
            trace.append(("len", s))
        length += src[s]
        s += 1
        if len(dst) + length > cap:
            paths["refuse_match_past_end"] += 1
            return False, b"", paths
        dist = len(dst) - ref
        paths["match"] += 1
        if nfe:
            paths["match_fe_run"] += 1
        if dist < length:
            paths["match_overlap"] += 1
            unit = bytes(dst[ref:])
            dst += (unit * (length // dist + 1))[:length]
        else:
            dst += dst[ref:ref + length]
        ctx = le32(dst, len(dst) - 4)
    return True, bytes(dst), paths
