"""Many independent streams in one device call (knz_hip_encode_streams / knz_hip_decode_streams, csrc/streams.hip): every stream of a
batch must be the file the unmodified reference (oracle/_ref) writes for that item alone, lie at a 16-byte boundary with zeros up to
the next, equal what knz_hip_encode_blocks writes for the item, and come back through one decode call -- also beside damaged
neighbours, which get the verdict a single-stream call gives them and change no byte outside their own room."""
import importlib

import numpy as np
import pytest

import knzlib
import vectors

pytestmark = pytest.mark.gpu

BS = 1024
FILL = 0xA5
_ref = []
_pool = {}


def reference():
    """The reference build. Its absence is a failure, not a skip."""
    if not _ref:
        _ref.append(knzlib.Ref())
    return _ref[0]


def mods():
    knzlib.load_pkg()
    return importlib.import_module("kanzi_amd.hipapi"), importlib.import_module("kanzi_amd.framing")


def pool(kind):
    """One long buffer per generator of tests/vectors.py; the items are slices of it."""
    if kind not in _pool:
        spec = {"text": ("text", 200000, 1), "mixed": ("mixed", 200000, 2), "runs": ("runs", 40, 9000), "rand": ("rand", 200000, 7)}[kind]
        _pool[kind] = vectors.make(spec)
    return _pool[kind]


def small_items(n_extra=300, seed=5):
    """The lengths the issue names -- empty, copy blocks (<= 15), 16, one byte around the block size (1025: a second block that is a
    1-byte copy block), three blocks and a tail -- and n_extra more of 0..2000 bytes: more streams than a wave and than a workgroup of 256
    threads, stream lengths of every residue mod 16."""
    rng = np.random.default_rng(seed)
    items = [pool("text")[1000:1000 + n] for n in (0, 1, 15, 16, 1023, 1024, 1025, 3 * 1024 + 77)]
    kinds = ("text", "mixed", "runs", "rand")
    for k in range(n_extra):
        n = int(rng.integers(0, 2001))
        src = pool(kinds[k % 4])
        at = int(rng.integers(0, len(src) - n))
        items.append(src[at:at + n])
    return items


def round16(v):
    return (v + 15) & ~15


def pack(buffers):
    """The buffers one behind the other, each at a multiple of 16: (bytes, offsets)."""
    blob, offs = bytearray(), []
    for b in buffers:
        blob += bytes(-len(blob) % 16)
        offs.append(len(blob))
        blob += b
    return bytes(blob) + bytes(64), offs


def encode_batch(hip, items, transform, entropy, checksum=0, jobs=1, bs=BS):
    """One knz_hip_encode_streams call, every stream with its own header in front. Returns the streams, and checks how they lie."""
    hipapi, framing = mods()
    p = hip.params(transform, entropy, bs, checksum, jobs)
    blob, offs = pack(items)
    arr = (hipapi.Item * len(items))()
    pro = bytearray()
    for i, it in enumerate(items):
        h, hb = framing.make_header(p.entropy_type, p.transform_type, bs, checksum, len(it))
        arr[i].in_off, arr[i].in_len, arr[i].prologue_off, arr[i].prologue_bits = offs[i], len(it), len(pro), hb
        pro += h
    cap = hip.encode_streams_bound(p, arr)
    if p.entropy_type in hipapi.BINARY_CODERS:
        cap += 32 * len(blob)               # the bound is these coders' first tier (include/knz_hip.h)
    d_in, d_out = hip.malloc(len(blob)), hip.malloc(cap)
    try:
        hip.h2d(d_in, blob)
        hip.h2d(d_out, bytes([FILL]) * cap)                     # the call clears what it uses
        used = hip.encode_streams(p, d_in, arr, d_out, cap, prologues=bytes(pro))
        raw = hip.d2h(d_out, used)
    finally:
        hip.free(d_in)
        hip.free(d_out)
    streams, at = [], 0
    for i, it in enumerate(items):
        assert arr[i].error == 0 and arr[i].blocks == (len(it) + bs - 1) // bs, i
        assert arr[i].out_off % 16 == 0 and arr[i].out_off == at, (i, arr[i].out_off, at)
        nbytes = (arr[i].out_len + 7) // 8
        streams.append(raw[at:at + nbytes])
        assert raw[at + nbytes:round16(at + nbytes)] == bytes(round16(at + nbytes) - at - nbytes), "padding behind stream %d is not zero" % i
        at = round16(at + nbytes)
    assert used == at
    return streams


def encode_single(hip, item, transform, entropy, checksum=0, jobs=1, bs=BS):
    hipapi, framing = mods()
    p = hip.params(transform, entropy, bs, checksum, jobs)
    h, hb = framing.make_header(p.entropy_type, p.transform_type, bs, checksum, len(item))
    cap = hip.encode_bound(p, len(item)) + 64 + (32 * len(item) if p.entropy_type in hipapi.BINARY_CODERS else 0)
    d_in, d_out = hip.malloc(len(item) + 64), hip.malloc(cap)
    try:
        if item:
            hip.h2d(d_in, item)
        bits = hip.encode_blocks(p, d_in, len(item), d_out, cap, prologue=h, prologue_bits=hb)
        return hip.d2h(d_out, (bits + 7) // 8)
    finally:
        hip.free(d_in)
        hip.free(d_out)


def decode_batch(hip, streams, caps, in_bits=None, guard=48):
    """One knz_hip_decode_streams call over streams of one header. Every item's room lies `guard` bytes (and up to the next multiple of
    16) behind the one before, in a buffer filled with a pattern. Returns (items, the whole output buffer, the rooms' offsets)."""
    hipapi, framing = mods()
    hdr = framing.parse_header(streams[0])
    p = hip.params(hdr["ttype"], hdr["etype"], hdr["block_size"], hdr["checksum_bits"], 1, hdr["bs_version"])
    blob, offs = pack(streams)
    arr = (hipapi.Item * len(streams))()
    at, outs = round16(guard), []
    for i, s in enumerate(streams):
        arr[i].in_off, arr[i].in_len = offs[i], (8 * len(s) if in_bits is None or in_bits[i] is None else in_bits[i])
        arr[i].start_bit = framing.parse_header(s)["bits"]
        arr[i].out_off, arr[i].out_cap = at, caps[i]
        outs.append(at)
        at = round16(at + caps[i] + guard)
    total = at + 64
    d_in, d_out = hip.malloc(len(blob)), hip.malloc(total)
    try:
        hip.h2d(d_in, blob)
        hip.h2d(d_out, bytes([FILL]) * total)
        hip.decode_streams(p, d_in, arr, d_out, total)
        return arr, hip.d2h(d_out, total), outs
    finally:
        hip.free(d_in)
        hip.free(d_out)


def decode_single(hip, stream, cap, in_bits=None):
    """knz_hip_decode_blocks on one stream alone: (error code or 0, bytes)."""
    hipapi, framing = mods()
    hdr = framing.parse_header(stream)
    p = hip.params(hdr["ttype"], hdr["etype"], hdr["block_size"], hdr["checksum_bits"], 1, hdr["bs_version"])
    d_in, d_out = hip.malloc(len(stream) + 64), hip.malloc(cap + 64)
    try:
        hip.h2d(d_in, stream + bytes(64))
        try:
            n, _, _ = hip.decode_blocks(p, d_in, 8 * len(stream) if in_bits is None else in_bits, hdr["bits"], d_out, cap)
        except hipapi.KnzError as e:
            return e.code, b""
        return 0, hip.d2h(d_out, n)
    finally:
        hip.free(d_in)
        hip.free(d_out)


def typed_items():
    """A batch whose blocks get different data types from their first bytes: a WAV header, DNA, text -- and the small lengths."""
    c = knzlib.corpus()
    wav = b"RIFF" + (36 + 3000).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + bytes([1, 0, 2, 0, 0x44, 0xAC, 0, 0, 0x10, 0xB1, 2, 0, 4, 0, 16, 0]) + b"data" + (3000).to_bytes(4, "little") + pool("rand")[:3000]
    # (wav[:1500] ends in a block of 476 bytes whose RANGE stream the reference writes and cannot read: such an item must get its
    # verdict in a batch like anywhere else, test_batch_equals_reference_and_single_calls)
    out = [wav, c.dna(2500, 4), pool("text")[:2100], c.dna(1024, 5), wav[:1500], pool("text")[5000:5300], wav[:1600]]
    return out + small_items(40, seed=8)


CHAINS = [
    # (transform, entropy, checksum, items)
    ("NONE", "NONE", 0, "small"),                             # the direct path
    ("BWT+MTFT+ZRLT", "ANS0", 32, "small"),
    ("LZX", "HUFFMAN", 64, "small"),
    ("RLT", "FPAQ", 0, "small"),
    ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0", 0, "small"),           # five stages: the skip byte
    ("PACK", "RANGE", 0, "typed"),                            # the data type per block
    ("LZP", "CM", 0, "small"),
    ("RLT", "TPAQ", 0, "few"),
    ("RLT", "ANS1", 32, "small"),                             # metadata per decode lane
    ("RLT", "TPAQX", 0, "few"),                               # tables per decode lane
]


@pytest.mark.parametrize("transform,entropy,checksum,which", CHAINS, ids=[c[0] + "/" + c[1] for c in CHAINS])
def test_batch_equals_reference_and_single_calls(hip, transform, entropy, checksum, which):
    items = small_items() if which == "small" else small_items(12) if which == "few" else typed_items()
    ref = reference()
    streams = encode_batch(hip, items, transform, entropy, checksum)
    unreadable = {}                                            # streams the reference writes and cannot read itself
    for i, it in enumerate(items):
        rc, want = ref.compress(it, transform, entropy, BS, checksum=checksum, orig_size=len(it))
        assert rc == 0
        assert streams[i] == want, "stream %d (%d bytes) differs from the reference's" % (i, len(it))
        rc, back = ref.decompress(want, len(it) + BS)
        if rc != 0 or back != it:
            unreadable[i] = decode_single(hip, want, round16(len(it)))[0]
            assert unreadable[i] != 0, i
    assert len(unreadable) == (1 if which == "typed" else 0), unreadable
    if which == "small":
        assert {len(s) % 16 for s in streams} == set(range(16))
        assert len(items) > 256
    for i, it in enumerate(items):
        assert encode_single(hip, it, transform, entropy, checksum) == streams[i], "stream %d differs from knz_hip_encode_blocks'" % i
    # the way back in one call, as one range of blocks and as three
    for parts in (1, 3):
        assert hip.L.knz_hip_tune(b"dec_parts", parts) == 0
        try:
            arr, raw, outs = decode_batch(hip, streams, [round16(len(it)) for it in items])
        finally:
            hip.L.knz_hip_tune(b"dec_parts", 3)
        for i, it in enumerate(items):
            if i in unreadable:
                assert arr[i].error == unreadable[i] and arr[i].out_len == 0, (parts, i, arr[i].error)
                continue
            assert arr[i].error == 0 and arr[i].out_len == len(it) and arr[i].blocks == (len(it) + BS - 1) // BS, (parts, i, arr[i].error)
            assert raw[outs[i]:outs[i] + len(it)] == it, (parts, i)


def test_jobs_capacity_corner(hip):
    """knz_params.jobs: the buffer a block sees depends on its id inside ITS stream (i % jobs). ZRLT on data it expands, 1-4 blocks."""
    rng = np.random.default_rng(3)
    grow = rng.choice(np.array([0xFE, 0xFF, 0x80, 0x81, 0xF0], dtype=np.uint8), size=6000).tobytes()      # no zeros, many escapes
    items = [grow[a:a + n] for a, n in ((0, 1024), (100, 2048), (200, 3 * 1024), (300, 4 * 1024), (10, 4 * 1024 - 5), (20, 2 * 1024 + 1), (30, 700), (40, 3 * 1024 + 15),
                                                (50, 1024 + 300), (60, 2048 + 500), (70, 1024 + 700))]      # (short last blocks with ids 1 and 2: their buffers differ)
    ref = reference()
    streams = encode_batch(hip, items, "ZRLT", "HUFFMAN", 0, jobs=3)
    differs = 0
    for i, it in enumerate(items):
        rc, want = ref.compress(it, "ZRLT", "HUFFMAN", BS, jobs=3, orig_size=len(it))
        assert rc == 0 and streams[i] == want, i
        differs += want != ref.compress(it, "ZRLT", "HUFFMAN", BS, jobs=1, orig_size=len(it))[1]
    assert differs, "the job count changes no stream of this batch: the case tests nothing"


def flip(stream, bit):
    b = bytearray(stream)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def bits_at(stream, pos, n):
    return (int.from_bytes(stream[pos >> 3:(pos >> 3) + 8].ljust(8, b"\0"), "big") >> (64 - (pos & 7) - n)) & ((1 << n) - 1)


def test_damaged_items_stay_alone(hip):
    hipapi, framing = mods()
    transform, entropy, checksum = "BWT+MTFT+ZRLT", "ANS0", 32
    items = small_items(40, seed=11)
    good = encode_batch(hip, items, transform, entropy, checksum)
    hbs = [framing.parse_header(s)["bits"] for s in good]      # (the header's size field has the width the size needs)
    long_ones = [i for i, it in enumerate(items) if len(it) > 2 * BS] + [i for i, it in enumerate(items) if BS < len(it) <= 2 * BS]
    mid = [i for i, it in enumerate(items) if 100 < len(it) < BS]
    streams, caps, in_bits = list(good), [round16(len(it)) for it in items], [None] * len(items)
    a, b, c, d = mid[0], mid[1], long_ones[0], mid[2]
    lw = bits_at(good[a], hbs[a], 5) + 3
    streams[a] = flip(good[a], hbs[a] + 5 + 1)                 # a bit of the first block's length
    in_bits[b] = hbs[b] + (8 * len(good[b]) - hbs[b]) // 2     # truncated
    caps[c] = round16(len(items[c]) - BS - 16)                 # one block short
    lw_d = bits_at(good[d], hbs[d], 5) + 3                     # wrong stored checksum of the first block
    mode = bits_at(good[d], hbs[d] + 5 + lw_d, 8)
    assert not (mode & 0x80) and not (mode & 0x10) and lw >= 4
    streams[d] = flip(good[d], hbs[d] + 5 + lw_d + 8 + 8 * (1 + ((mode >> 5) & 3)) + 31)
    damaged = {a, b, c, d}
    want = {i: decode_single(hip, streams[i], caps[i], in_bits[i])[0] for i in damaged}
    assert all(want.values()), want
    assert want[d] == 19 and want[b] == 11, want              # KNZ_ERR_CRC_CHECK, KNZ_ERR_READ_FILE
    arr, raw, outs = decode_batch(hip, streams, caps, in_bits)
    clean, raw_clean, outs_clean = decode_batch(hip, [s for i, s in enumerate(good) if i not in damaged], [cp for i, cp in enumerate(caps) if i not in damaged])
    k = 0
    for i, it in enumerate(items):
        if i in damaged:
            assert arr[i].error == want[i] and arr[i].out_len == 0, (i, arr[i].error, want[i])
            continue
        assert arr[i].error == 0 and arr[i].out_len == len(it) and raw[outs[i]:outs[i] + len(it)] == it, i
        # ... exactly as a call without the damaged items leaves it
        assert (clean[k].error, clean[k].out_len, clean[k].blocks) == (arr[i].error, arr[i].out_len, arr[i].blocks)
        assert raw_clean[outs_clean[k]:outs_clean[k] + caps[i]] == raw[outs[i]:outs[i] + caps[i]], i
        k += 1
    # nothing outside the items' rooms has changed
    mask = np.ones(len(raw), dtype=bool)
    for i in range(len(items)):
        mask[outs[i]:outs[i] + caps[i]] = False
    assert (np.frombuffer(raw, dtype=np.uint8)[mask] == FILL).all()


def test_calls_refused_as_a_whole(hip):
    hipapi, framing = mods()
    items = small_items(6, seed=2)
    blob, offs = pack(items)
    d_in, d_out = hip.malloc(len(blob)), hip.malloc(1 << 20)
    try:
        hip.h2d(d_in, blob)

        def call(transform="NONE", entropy="ANS0", shift=0, short=0):
            p = hip.params(transform, entropy, BS)
            arr = (hipapi.Item * len(items))()
            for i, it in enumerate(items):
                arr[i].in_off, arr[i].in_len = offs[i] + (shift if i == 3 else 0), len(it)
            cap = hip.encode_streams_bound(p, arr)
            assert cap <= 1 << 20
            return hip.encode_streams(p, d_in, arr, d_out, cap - short), arr

        with pytest.raises(hipapi.KnzError, match="multiple of 16") as e:
            call(shift=8)
        assert e.value.code == 18
        with pytest.raises(hipapi.KnzError, match="LZ / LZX behind PACK") as e:
            call(transform="PACK+LZ")
        assert e.value.code == 3
        with pytest.raises(hipapi.KnzError, match="output buffer too small") as e:
            call(short=1)
        assert e.value.code == 12
        # the context is as usable as before
        used, arr = call()
        raw = hip.d2h(d_out, used)
        ref = reference()
        for i, it in enumerate(items):
            rc, want = ref.compress(it, "NONE", "ANS0", BS, headerless=1)
            assert rc == 0 and raw[arr[i].out_off:arr[i].out_off + (arr[i].out_len + 7) // 8] == want, i
    finally:
        hip.free(d_in)
        hip.free(d_out)


def test_compress_many_round_trip(hip):
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    framing = importlib.import_module("kanzi_amd.framing")
    items = small_items(38, seed=4)[6:]                        # 40 buffers: an empty one is among the random lengths or added here
    items[0], items[1] = b"", pool("mixed")[:2 * BS + 300]
    assert len(items) == 40
    ref = reference()
    for transform, entropy, checksum in (("BWT+MTFT+ZRLT", "ANS0", 32), ("LZX", "HUFFMAN", 0)):
        streams = kz.compress_many(items, transform, entropy, BS, checksum=checksum)
        for i, it in enumerate(items):
            rc, want = ref.compress(it, transform, entropy, BS, checksum=checksum, orig_size=len(it))
            assert rc == 0 and streams[i] == want, (transform, i)
        assert kz.decompress_many(streams) == items
        # a stream without a stored size goes through the single-stream path
        rc, nosize = ref.compress(items[1], transform, entropy, BS, checksum=checksum, orig_size=0)
        assert rc == 0 and framing.parse_header(nosize)["orig_size"] == 0
        mixed = [streams[5], nosize, streams[0], ref.compress(items[7], "RLT", "FPAQ", 4096, orig_size=len(items[7]))[1]]
        assert kz.decompress_many(mixed) == [items[5], items[1], items[0], items[7]]


def test_many_small_items_under_a_large_block_size(hip):
    """650 items of at most 2,000 bytes in streams of 4 MiB blocks (the CLI's default): a call is sized by what its items hold, not by the
    block size of their format -- by the block size, 512 one-block items would already be the 2 GiB of a call, and far fewer would take
    gigabytes of workspace. Through the C ABI, and through compress_many / decompress_many with one buffer of more than a block among
    the small ones, which the Python layer has to keep out of the small ones' call (blocks x longest block)."""
    knzlib.load_pkg()
    kz = importlib.import_module("kanzi_amd.kanzi")
    big_bs = 4 << 20
    items = small_items(642, seed=21)
    assert len(items) == 650
    ref = reference()
    for transform, entropy, checksum in (("BWT+RANK+ZRLT", "ANS0", 32), ("LZX", "HUFFMAN", 0)):
        want = []
        for it in items:
            rc, w = ref.compress(it, transform, entropy, big_bs, checksum=checksum, orig_size=len(it))
            assert rc == 0
            want.append(w)
        assert encode_batch(hip, items, transform, entropy, checksum, bs=big_bs) == want, transform
        arr, raw, outs = decode_batch(hip, want, [round16(len(it)) for it in items])
        for i, it in enumerate(items):
            assert arr[i].error == 0 and arr[i].out_len == len(it) and raw[outs[i]:outs[i] + len(it)] == it, (transform, i, arr[i].error)
        assert kz.compress_many(items, transform, entropy, big_bs, checksum=checksum) == want, transform
        assert kz.decompress_many(want) == items, transform
    # one buffer of a block and a bit among them
    large = pool("mixed")[:150000] * 28 + pool("text")[:100]
    assert len(large) > big_bs
    mix = items[:325] + [large] + items[325:]
    streams = kz.compress_many(mix, "LZX", "HUFFMAN", big_bs)
    rc, w = ref.compress(large, "LZX", "HUFFMAN", big_bs, orig_size=len(large))
    assert rc == 0 and streams[325] == w and streams[:325] + streams[326:] == want
    assert kz.decompress_many(streams) == mix
    # a stream that ends before the size its header promises is an error, not a short result
    framing = importlib.import_module("kanzi_amd.framing")
    p = hip.params("LZX", "HUFFMAN", big_bs)
    h, hb = framing.make_header(p.entropy_type, p.transform_type, big_bs, 0, len(items[7]) + 1000)
    assert hb % 8 == 0
    lying = h + want[7][framing.parse_header(want[7])["bits"] // 8:]
    with pytest.raises(kz.KanziError) as e:
        kz.decompress_many([want[3], lying])
    assert e.value.code == 13


def test_a_call_over_the_work_limit_is_refused_by_name(hip):
    """blocks x longest block above the limit: the call fails as a whole and says what to do; the context stays usable."""
    hipapi, framing = mods()
    items = [(pool("rand") * 6)[:1 << 20]] + [b"x" * 20] * 4500              # 4,501 blocks, the longest of 1 MiB: 4.4 GiB of workspace
    with pytest.raises(hipapi.KnzError, match="split the call") as e:
        encode_batch(hip, items, "NONE", "NONE", bs=1 << 20)
    assert e.value.code == 18
    assert encode_batch(hip, items[1:9], "NONE", "NONE", bs=1 << 20)
