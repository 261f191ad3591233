"""Edges of the batch encode and decode drivers (csrc/api.hip) that no other file asserts: the refusals knz_hip_encode_blocks makes before
it launches anything, an empty input with and without a prologue, a table of streams whose blocks take the binary coders' second
staging tier, and a damaged block in the middle of a batch that is decoded in three ranges. Everything goes through the C ABI
(kanzi-cpp_amd/hipapi.py); the streams' helpers are those of tests/test_gpu_streams.py."""
import importlib

import numpy as np
import pytest

import knzlib
import test_gpu_streams as ts

pytestmark = pytest.mark.gpu

ERR_WRITE_FILE, ERR_PROCESS_BLOCK, ERR_INVALID_PARAM, ERR_CRC_CHECK = 12, 13, 18, 19
FILL = 0xA5


def _hipapi():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.hipapi")


def test_encode_refusals_leave_the_context_usable(hip, oracle):
    """Each refusal by code and message; after each one the same context encodes the batch to the oracle's bytes."""
    hipapi = _hipapi()
    bs = 1024
    data = knzlib.corpus().mixed(4096, 2)
    rc, want = oracle.compress(data, "NONE", "ANS0", bs, headerless=1)
    assert rc == 0
    p = hip.params("NONE", "ANS0", bs)
    cap = hip.encode_bound(p, len(data))
    d_in, d_out = hip.malloc(len(data) + 64), hip.malloc(cap)
    try:
        hip.h2d(d_in, data + bytes(64))

        def refused(code, fragment, **kw):
            args = dict(p=p, d_in=d_in, out_cap=cap, prologue=b"", prologue_bits=0)
            args.update(kw)
            with pytest.raises(hipapi.KnzError, match=fragment) as e:
                hip.encode_blocks(args["p"], args["d_in"], len(data), d_out, args["out_cap"], prologue=args["prologue"], prologue_bits=args["prologue_bits"])
            assert e.value.code == code, (fragment, e.value.code)
            bits = hip.encode_blocks(p, d_in, len(data), d_out, cap)
            assert hip.d2h(d_out, (bits + 7) // 8) == want, fragment

        refused(ERR_INVALID_PARAM, "16-byte aligned", d_in=d_in + 8)
        refused(ERR_INVALID_PARAM, "invalid block size", p=hip.params("NONE", "ANS0", 1000))
        refused(ERR_INVALID_PARAM, "invalid block size", p=hip.params("NONE", "ANS0", 1032))
        refused(ERR_INVALID_PARAM, "prologue too long", prologue=bytes(201), prologue_bits=1608)
        refused(ERR_WRITE_FILE, "output buffer too small", out_cap=16)
    finally:
        hip.free(d_in)
        hip.free(d_out)


def test_empty_input(hip):
    """n = 0: the prologue's bits and, with finish, the 8 bits of the end marker; the bytes are the prologue followed by zeros."""
    pro = bytes([0xC3, 0x5A, 0x96, 0xF1, 0xB8])                # 37 bits: the last byte's low three bits are no part of it
    p = hip.params("NONE", "ANS0", 1024)
    d_in, d_out = hip.malloc(64), hip.malloc(256)
    try:
        for prologue, pbits, finish, bits in ((pro, 37, 1, 45), (pro, 37, 0, 37), (b"", 0, 1, 8)):
            hip.h2d(d_out, bytes([FILL]) * 256)
            assert hip.encode_blocks(p, d_in, 0, d_out, 256, prologue=prologue, prologue_bits=pbits, finish=finish) == bits
            assert hip.d2h(d_out, 8) == prologue + bytes(8 - len(prologue)), (pbits, finish)
    finally:
        hip.free(d_in)
        hip.free(d_out)


def test_streams_through_the_second_tier(hip, monkeypatch):
    """knz_hip_encode_streams with CM and the first tier lowered to n / 4 (KNZ_CM_TIER1_DIV, as tests/test_gpu_cm.py): an empty item, 4,096
    + 17 random bytes and 8,192 bytes of text in blocks of 4,096. The first staging of a block is 4,096 / 4 + 64 = 1,088 bytes; the random
    block codes to 4,161 bytes and, by tests/cm_model.py, the two text blocks to 2,201 and 2,197, so all three are coded a second time
    and the lengths of the whole table are summed and scanned again, while the 17-byte block (24 bytes) stays in the first tier. Every
    stream is what knz_hip_encode_blocks writes for the item alone, and one knz_hip_decode_streams call gives the inputs back."""
    monkeypatch.setenv("KNZ_CM_TIER1_DIV", "4")
    bs = 4096
    items = [b"", np.random.default_rng(17).integers(0, 256, bs + 17, dtype=np.uint8).tobytes(), knzlib.corpus().text(2 * bs, 3)]
    hip.set_profiling(True)
    try:
        streams = ts.encode_batch(hip, items, "NONE", "CM", bs=bs)           # (its output buffer: the bound plus 32 bytes per byte)
        launches = sum(k[2] for k in hip.kernel_times() if k[0] == "k_cm_encode")
    finally:
        hip.set_profiling(False)
    assert launches >= 2
    for i, it in enumerate(items):
        assert ts.encode_single(hip, it, "NONE", "CM", bs=bs) == streams[i], i
    arr, raw, outs = ts.decode_batch(hip, streams, [ts.round16(len(it)) for it in items])
    for i, it in enumerate(items):
        assert arr[i].error == 0 and arr[i].out_len == len(it) and arr[i].blocks == (len(it) + bs - 1) // bs, (i, arr[i].error)
        assert raw[outs[i]:outs[i] + len(it)] == it, i


def _block_spans(stream, start_bit):
    """(first bit, bits) of every block's body behind its length prefix (5 b lw - 3 | lw b length), up to the end marker."""
    total, nbits = int.from_bytes(stream, "big"), 8 * len(stream)

    def get(pos, n):
        return (total >> (nbits - pos - n)) & ((1 << n) - 1)

    spans, pos = [], start_bit
    while True:
        lw = get(pos, 5) + 3
        written = get(pos + 5, lw)
        if written == 0:
            return spans
        spans.append((pos + 5 + lw, written))
        pos += 5 + lw + written


def test_damaged_middle_block_with_lanes(hip, oracle):
    """Seven blocks of 1,024 bytes, BWT+MTFT+ZRLT / ANS0, decoded as three ranges (3 + 2 + 2 blocks): one byte a quarter into the entropy
    payload of block 4, the first of the second range, is inverted. The framing stays valid; the oracle's decoder gives up at that block
    with code 13, and so must the call, naming the block. The context decodes the undamaged stream afterwards, and as two items of one
    knz_hip_decode_streams call only the damaged one fails."""
    hipapi = _hipapi()
    framing = importlib.import_module("kanzi_amd.framing")
    bs, chain, entropy = 1024, "BWT+MTFT+ZRLT", "ANS0"
    data = knzlib.corpus().mixed(7 * bs, 2)
    rc, good = oracle.compress(data, chain, entropy, bs, orig_size=len(data))
    assert rc == 0
    hbits = framing.parse_header(good)["bits"]
    spans = _block_spans(good, hbits)
    assert len(spans) == 7
    first, written = spans[3]
    mode = ts.bits_at(good, first, 8)
    assert not (mode & 0x80)                                   # no copy block: mode byte, 1-4 length bytes, then the payload
    head = 8 + 8 * (1 + ((mode >> 5) & 3))
    at = (first + head + (written - head) // 4) // 8 + 1
    assert first + head <= 8 * at and 8 * at + 8 <= first + written
    bad = bytearray(good)
    bad[at] ^= 0xFF
    bad = bytes(bad)
    assert _block_spans(bad, hbits) == spans
    rc, back = oracle.decompress(bad, len(data) + bs)
    assert rc == ERR_PROCESS_BLOCK and back[:3 * bs] == data[:3 * bs]       # the reference's decoder reports the block, no silent miss
    p = hip.params(chain, entropy, bs)
    d_in, d_out = hip.malloc(len(good) + 64), hip.malloc(len(data) + bs + 64)
    assert hip.L.knz_hip_tune(b"dec_parts", 3) == 0
    try:
        hip.h2d(d_in, bad + bytes(64))
        with pytest.raises(hipapi.KnzError, match=r"block 4: decoding failed \(code 13\)") as e:
            hip.decode_blocks(p, d_in, 8 * len(bad), hbits, d_out, len(data) + bs)
        assert e.value.code == ERR_PROCESS_BLOCK
        hip.h2d(d_in, good + bytes(64))
        n, _, nb = hip.decode_blocks(p, d_in, 8 * len(good), hbits, d_out, len(data) + bs)
        assert nb == 7 and hip.d2h(d_out, n) == data
        for order in ((bad, good), (good, bad)):
            arr, raw, outs = ts.decode_batch(hip, list(order), [len(data), len(data)])
            for i, s in enumerate(order):
                if s is bad:
                    assert arr[i].error == ERR_PROCESS_BLOCK and arr[i].out_len == 0, (i, arr[i].error)
                else:
                    assert arr[i].error == 0 and arr[i].out_len == len(data) and arr[i].blocks == 7, (i, arr[i].error)
                    assert raw[outs[i]:outs[i] + len(data)] == data, i
    finally:
        hip.free(d_in)
        hip.free(d_out)
