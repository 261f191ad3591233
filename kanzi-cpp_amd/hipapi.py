"""ctypes binding of the device C-ABI (include/knz_hip.h, built into kanzi-cpp_amd/libknz_hip.so).

This module is the Python-side counterpart of the reference's src/api/kanzi_c_api.py for the
device layer: it only marshals pointers and sizes. There is no CPU fallback: if the library is
missing or no GPU is visible, calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libknz_hip.so")

E_NONE, E_HUFFMAN, E_FPAQ, E_RANGE, E_ANS0, E_CM, E_TPAQ, E_ANS1, E_TPAQX = 0, 1, 2, 4, 5, 6, 7, 8, 9
BINARY_CODERS = (E_CM, E_TPAQ, E_TPAQX)          # knz_hip_encode_bound is a first tier for these (include/knz_hip.h)
ENTROPY_IDS = {"NONE": 0, "HUFFMAN": 1, "FPAQ": 2, "RANGE": 4, "ANS0": 5, "CM": 6, "TPAQ": 7, "ANS1": 8, "TPAQX": 9}
TRANSFORM_IDS = {"NONE": 0, "BWT": 1, "BWTS": 2, "LZ": 3, "RLT": 5, "ZRLT": 6, "MTFT": 7, "RANK": 8, "EXE": 9, "TEXT": 10, "ROLZX": 12, "SRT": 13, "LZP": 14, "MM": 15, "LZX": 16, "UTF": 17, "PACK": 18, "DNA": 19, "TIMESTAMP": 64}

SYMBOLS = [
    "knz_hip_device_count", "knz_hip_create", "knz_hip_destroy", "knz_hip_last_error", "knz_hip_encode_bound",
    "knz_hip_encode_blocks", "knz_hip_decode_blocks", "knz_hip_entropy_encode", "knz_hip_entropy_decode",
    "knz_hip_transform_forward", "knz_hip_transform_forward_dt", "knz_hip_transform_inverse", "knz_hip_malloc", "knz_hip_free",
    "knz_hip_memcpy_h2d", "knz_hip_memcpy_d2h", "knz_hip_sync", "knz_hip_memcpy_h2d_async", "knz_hip_memcpy_d2h_async", "knz_hip_copy_wait", "knz_hip_host_alloc", "knz_hip_host_free", "knz_hip_set_profiling", "knz_hip_get_kernel_times",
    "knz_hip_tune", "knz_hip_transform_supported", "knz_hip_shift_bits", "knz_hip_encode_block_hosted", "knz_hip_decode_block_hosted",
    "knz_hip_entropy_decode_v", "knz_hip_transform_inverse_v", "knz_hip_range_divide",
    "knz_hip_entropy_encode_bs", "knz_hip_entropy_decode_bs", "knz_hip_tpaq_params",
    "knz_hip_transform_forward_bs", "knz_hip_transform_inverse_bs",
    "knz_hip_prims_info", "knz_hip_prims_scan", "knz_hip_prims_sort",
    "knz_hip_encode_streams_bound", "knz_hip_encode_streams", "knz_hip_decode_streams", "knz_hip_copy_many",
    "knz_hip_split_many", "knz_hip_join_many",
]
STREAMS_MAX_ITEMS = STREAMS_MAX_BLOCKS = 65536      # KNZ_STREAMS_MAX_ITEMS / _BLOCKS of include/knz_hip.h
BATCH_MAX_BYTES = 0x7FFFFFFF                        # input of one encode call, decoded bytes of one decode call
COPY_MAX_COPIES = 1 << 20                           # KNZ_COPY_MAX_COPIES


class Params(C.Structure):
    _fields_ = [("transform_type", C.c_uint64), ("entropy_type", C.c_int32), ("block_size", C.c_int32),
                ("checksum_bits", C.c_int32), ("jobs", C.c_int32), ("bs_version", C.c_int32)]


class Item(C.Structure):
    """knz_item: one stream of a knz_hip_encode_streams / knz_hip_decode_streams call."""
    _fields_ = [("in_off", C.c_uint64), ("in_len", C.c_uint64), ("start_bit", C.c_uint64), ("prologue_off", C.c_uint32),
                ("prologue_bits", C.c_uint32), ("out_off", C.c_uint64), ("out_cap", C.c_uint64), ("out_len", C.c_uint64),
                ("blocks", C.c_int32), ("error", C.c_int32)]


class Copy(C.Structure):
    """knz_copy: one copy of a knz_hip_copy_many call (device addresses, bytes)."""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("len", C.c_uint64)]


class PlaneCopy(C.Structure):
    """knz_plane_copy: one entry of a knz_hip_split_many / knz_hip_join_many call (device addresses, bytes, bytes per element)."""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("len", C.c_uint64), ("elem", C.c_uint32), ("reserved", C.c_uint32)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_float), ("launches", C.c_uint64)]


class KnzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("knz_hip error %d: %s" % (code, msg))
        self.code = code


def transform_type(names):
    """TransformFactory::getType (transform/TransformFactory.hpp:100-137): 6 bits per stage, NONE dropped."""
    res, shift = 0, 42
    toks = names.upper().split("+")
    if len(toks) > 8:
        raise ValueError("Only 8 transforms allowed")
    if len(toks) == 1:
        return TRANSFORM_IDS[toks[0]] << 42
    for t in toks:
        v = TRANSFORM_IDS[t]
        if v:
            res |= v << shift
            shift -= 6
    return res


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libknz_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        vp, u8p, sz = C.c_void_p, C.c_void_p, C.c_size_t
        L.knz_hip_device_count.argtypes = [C.POINTER(C.c_int)]
        L.knz_hip_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        L.knz_hip_destroy.argtypes = [vp]; L.knz_hip_destroy.restype = None
        L.knz_hip_last_error.argtypes = [vp]; L.knz_hip_last_error.restype = C.c_char_p
        L.knz_hip_encode_bound.argtypes = [C.POINTER(Params), sz]; L.knz_hip_encode_bound.restype = sz
        L.knz_hip_encode_blocks.argtypes = [vp, C.POINTER(Params), u8p, sz, C.c_char_p, C.c_uint32, C.c_int64, C.c_int,
                                            u8p, sz, C.POINTER(C.c_uint64)]
        L.knz_hip_decode_blocks.argtypes = [vp, C.POINTER(Params), u8p, C.c_uint64, C.c_uint64, C.c_int64, u8p, sz,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
        L.knz_hip_entropy_encode.argtypes = [vp, C.c_int, C.c_char_p, C.c_uint32, u8p, sz, C.POINTER(C.c_uint64)]
        L.knz_hip_entropy_decode.argtypes = [vp, C.c_int, C.c_char_p, C.c_uint64, C.c_uint64, u8p, C.c_uint32,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        L.knz_hip_entropy_decode_v.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_uint64, C.c_uint64, u8p, C.c_uint32,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        L.knz_hip_transform_inverse_v.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_int32, u8p, C.c_int32,
                                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.knz_hip_transform_forward.argtypes = [vp, C.c_int, C.c_char_p, C.c_int32, u8p, C.c_int32, C.c_int,
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.knz_hip_transform_inverse.argtypes = [vp, C.c_int, C.c_char_p, C.c_int32, u8p, C.c_int32,
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.knz_hip_transform_forward_dt.argtypes = [vp, C.c_int, C.c_char_p, C.c_int32, u8p, C.c_int32, C.c_int,
                                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.knz_hip_transform_forward_bs.argtypes = [vp, C.c_int, C.c_uint32, C.c_char_p, C.c_int32, u8p, C.c_int32, C.c_int,
                                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.knz_hip_transform_inverse_bs.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_char_p, C.c_int32, u8p, C.c_int32,
                                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.knz_hip_malloc.argtypes = [vp, sz, C.POINTER(vp)]
        L.knz_hip_free.argtypes = [vp, vp]
        L.knz_hip_memcpy_h2d.argtypes = [vp, vp, C.c_char_p, sz]
        L.knz_hip_memcpy_d2h.argtypes = [vp, vp, vp, sz]
        L.knz_hip_sync.argtypes = [vp]
        L.knz_hip_set_profiling.argtypes = [vp, C.c_int]
        L.knz_hip_get_kernel_times.argtypes = [vp, C.POINTER(KernelTime), C.c_int]
        L.knz_hip_tune.argtypes = [C.c_char_p, C.c_int]
        L.knz_hip_shift_bits.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, u8p]
        L.knz_hip_range_divide.argtypes = [vp, vp, vp, C.c_uint32, vp]
        L.knz_hip_entropy_encode_bs.argtypes = [vp, C.c_int, C.c_uint32, C.c_char_p, C.c_uint32, u8p, sz, C.POINTER(C.c_uint64)]
        L.knz_hip_entropy_decode_bs.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint64, u8p, C.c_uint32,
                                                C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        L.knz_hip_tpaq_params.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
        L.knz_hip_prims_info.argtypes = [C.POINTER(C.c_uint32)]
        L.knz_hip_prims_scan.argtypes = [vp, C.c_int, vp, vp, sz, vp, vp]
        L.knz_hip_prims_sort.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, sz, C.c_int, C.c_int, vp, vp]
        L.knz_hip_encode_streams_bound.argtypes = [C.POINTER(Params), C.POINTER(Item), sz]; L.knz_hip_encode_streams_bound.restype = sz
        L.knz_hip_encode_streams.argtypes = [vp, C.POINTER(Params), u8p, C.POINTER(Item), sz, C.c_char_p, C.c_int, u8p, sz, C.POINTER(C.c_uint64)]
        L.knz_hip_decode_streams.argtypes = [vp, C.POINTER(Params), u8p, C.POINTER(Item), sz, u8p, sz]
        L.knz_hip_copy_many.argtypes = [vp, C.POINTER(Copy), sz]
        L.knz_hip_split_many.argtypes = [vp, C.POINTER(PlaneCopy), sz]
        L.knz_hip_join_many.argtypes = [vp, C.POINTER(PlaneCopy), sz]
        _lib = L
    return _lib


class Context:
    """One device context (one per GPU / per process rank)."""

    def __init__(self, device=0, stream=None):
        L = lib()
        h = C.c_void_p()
        rc = L.knz_hip_create(device, C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != 0:
            raise KnzError(rc, "cannot create device context (no GPU visible?)")
        self.h = h
        self.L = L

    def close(self):
        if self.h:
            self.L.knz_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise KnzError(rc, self.L.knz_hip_last_error(self.h).decode())

    # ---- device memory
    def malloc(self, n):
        p = C.c_void_p()
        self._chk(self.L.knz_hip_malloc(self.h, n, C.byref(p)))
        return p.value

    def free(self, p):
        self._chk(self.L.knz_hip_free(self.h, C.c_void_p(p)))

    def h2d(self, dptr, data):
        self._chk(self.L.knz_hip_memcpy_h2d(self.h, C.c_void_p(dptr), data, len(data)))

    def d2h(self, dptr, n):
        buf = (C.c_uint8 * max(1, n))()
        self._chk(self.L.knz_hip_memcpy_d2h(self.h, buf, C.c_void_p(dptr), n))
        return C.string_at(buf, n)

    def sync(self):
        self._chk(self.L.knz_hip_sync(self.h))

    # ---- batch API on device pointers
    def params(self, transform, entropy, block_size, checksum=0, jobs=1, bs_version=0):
        p = Params()
        p.transform_type = transform_type(transform) if isinstance(transform, str) else transform
        p.entropy_type = ENTROPY_IDS[entropy.upper()] if isinstance(entropy, str) else entropy
        p.block_size = block_size
        p.checksum_bits = checksum
        p.jobs = jobs
        p.bs_version = bs_version
        return p

    def encode_bound(self, p, n):
        return self.L.knz_hip_encode_bound(C.byref(p), n)

    def encode_blocks(self, p, d_in, n, d_out, out_cap, prologue=b"", prologue_bits=0, first_block=0, finish=1):
        bits = C.c_uint64(0)
        self._chk(self.L.knz_hip_encode_blocks(self.h, C.byref(p), C.c_void_p(d_in), n, prologue, prologue_bits,
                                               first_block, finish, C.c_void_p(d_out), out_cap, C.byref(bits)))
        return bits.value

    def decode_blocks(self, p, d_in, in_bits, start_bit, d_out, out_cap, max_blocks=0):
        ob, eb, nb = C.c_uint64(0), C.c_uint64(0), C.c_int64(0)
        self._chk(self.L.knz_hip_decode_blocks(self.h, C.byref(p), C.c_void_p(d_in), in_bits, start_bit, max_blocks,
                                               C.c_void_p(d_out), out_cap, C.byref(ob), C.byref(eb), C.byref(nb)))
        return ob.value, eb.value, nb.value

    # ---- many streams in one call, on device pointers
    def encode_streams_bound(self, p, items):
        return self.L.knz_hip_encode_streams_bound(C.byref(p), items, len(items))

    def encode_streams(self, p, d_in, items, d_out, out_cap, prologues=b"", finish=1):
        """items: an array of Item (in_off, in_len, prologue_off, prologue_bits set); the call fills out_off, out_len (bits) and blocks.
        Returns the bytes of d_out in use."""
        used = C.c_uint64(0)
        self._chk(self.L.knz_hip_encode_streams(self.h, C.byref(p), C.c_void_p(d_in), items, len(items), prologues, finish,
                                                C.c_void_p(d_out), out_cap, C.byref(used)))
        return used.value

    def decode_streams(self, p, d_in, items, d_out, out_cap):
        """items: an array of Item (in_off, in_len in bits, start_bit, out_off, out_cap set); the call fills out_len (bytes), blocks and
        error per item. Raises only for a failure of the call itself."""
        self._chk(self.L.knz_hip_decode_streams(self.h, C.byref(p), C.c_void_p(d_in), items, len(items), C.c_void_p(d_out), out_cap))

    def copy_many(self, copies):
        """copies: an array of Copy, or a sequence of (src, dst, len) device addresses and byte counts: all of them in one kernel launch
        on the context's stream. Returns without waiting for it; the sequence may be reused at once."""
        if not isinstance(copies, C.Array):
            flat = [v for c in copies for v in c]
            copies = (Copy * (len(flat) // 3)).from_buffer_copy((C.c_uint64 * len(flat))(*flat)) if flat else (Copy * 0)()
        self._chk(self.L.knz_hip_copy_many(self.h, copies, len(copies)))

    @staticmethod
    def _plane_entries(entries):
        if isinstance(entries, C.Array):
            return entries
        arr = (PlaneCopy * len(entries))()
        for e, (src, dst, n, elem) in zip(arr, entries):
            e.src, e.dst, e.len, e.elem = src, dst, n, elem
        return arr

    def split_many(self, entries):
        """entries: an array of PlaneCopy, or a sequence of (src, dst, len, elem): every entry's len / elem elements of elem bytes split into
        elem byte planes, dst[k * (len / elem) + i] = src[i * elem + k], all entries in one kernel launch on the context's stream (elem 1:
        a plain copy). Returns without waiting for it."""
        entries = self._plane_entries(entries)
        self._chk(self.L.knz_hip_split_many(self.h, entries, len(entries)))

    def join_many(self, entries):
        """The way back of split_many: dst[i * elem + k] = src[k * (len / elem) + i]."""
        entries = self._plane_entries(entries)
        self._chk(self.L.knz_hip_join_many(self.h, entries, len(entries)))

    # ---- per-stage API on host buffers
    def entropy_encode(self, entropy, data, stream_block_size=0):
        """stream_block_size: the block size of the stream the buffer belongs to (TPAQ and TPAQX size their tables by it); 0 = the
        buffer's own length."""
        e = ENTROPY_IDS[entropy.upper()]
        # (RANGE: up to 28 bits per byte and a bit; CM, TPAQ, TPAQX: the format's ceiling of 32 bytes per byte -- knz_hip_encode_bound)
        cap = (34 if e in BINARY_CODERS else 4 if e == E_RANGE else 2) * len(data) + 65536
        out = (C.c_uint8 * cap)()
        bits = C.c_uint64(0)
        self._chk(self.L.knz_hip_entropy_encode_bs(self.h, e, stream_block_size, data, len(data), out, cap, C.byref(bits)))
        return C.string_at(out, (bits.value + 7) // 8), bits.value

    def entropy_decode(self, entropy, enc, n, start_bit=0, in_bits=None, bs_version=0, stream_block_size=0):
        e = ENTROPY_IDS[entropy.upper()]
        out = (C.c_uint8 * max(1, n))()
        dec, used = C.c_int32(0), C.c_uint64(0)
        if in_bits is None:
            in_bits = 8 * len(enc)
        self._chk(self.L.knz_hip_entropy_decode_bs(self.h, e, bs_version, stream_block_size, enc, in_bits, start_bit, out, n, C.byref(dec), C.byref(used)))
        return dec.value, C.string_at(out, n), used.value

    def transform_forward(self, transform, data, dst_cap, entropy=None):
        t = TRANSFORM_IDS[transform.upper()]
        out = (C.c_uint8 * (max(dst_cap, len(data)) + 2048))()
        ol, ok = C.c_int32(0), C.c_int32(0)
        e = ENTROPY_IDS[entropy.upper()] if entropy else -1
        self._chk(self.L.knz_hip_transform_forward(self.h, t, data, len(data), out, dst_cap, e, C.byref(ol), C.byref(ok)))
        return ok.value, C.string_at(out, ol.value)

    def transform_forward_dt(self, transform, data, dst_cap, data_type, entropy=None):
        """The forward stage with a Context data type: returns (ok, bytes, the data type the stage left)."""
        t = TRANSFORM_IDS[transform.upper()]
        out = (C.c_uint8 * (max(dst_cap, len(data)) + 2048))()
        ol, ok, dt = C.c_int32(0), C.c_int32(0), C.c_int32(data_type)
        e = ENTROPY_IDS[entropy.upper()] if entropy else -1
        self._chk(self.L.knz_hip_transform_forward_dt(self.h, t, data, len(data), out, dst_cap, e, C.byref(dt), C.byref(ol), C.byref(ok)))
        return ok.value, C.string_at(out, ol.value), dt.value

    def transform_forward_bs(self, transform, data, dst_cap, data_type, entropy, stream_block_size):
        """transform_forward_dt with the block size of the stream the block belongs to (TEXT sizes its hash map by it)."""
        t = TRANSFORM_IDS[transform.upper()]
        out = (C.c_uint8 * (max(dst_cap, len(data)) + 2048))()
        ol, ok, dt = C.c_int32(0), C.c_int32(0), C.c_int32(data_type)
        e = ENTROPY_IDS[entropy.upper()] if entropy else -1
        self._chk(self.L.knz_hip_transform_forward_bs(self.h, t, stream_block_size, data, len(data), out, dst_cap, e, C.byref(dt), C.byref(ol), C.byref(ok)))
        return ok.value, C.string_at(out, ol.value), dt.value

    def transform_inverse_bs(self, transform, data, dst_cap, entropy, stream_block_size, bs_version=0):
        """The inverse stage with the stream's entropy coder and block size (TEXT reads both)."""
        t = TRANSFORM_IDS[transform.upper()]
        out = (C.c_uint8 * (dst_cap + 64))()
        ol, ok = C.c_int32(0), C.c_int32(0)
        e = ENTROPY_IDS[entropy.upper()] if entropy else -1
        self._chk(self.L.knz_hip_transform_inverse_bs(self.h, t, bs_version, stream_block_size, e, data, len(data), out, dst_cap, C.byref(ol), C.byref(ok)))
        return ok.value, C.string_at(out, ol.value)

    def transform_inverse(self, transform, data, dst_cap, bs_version=0):
        t = TRANSFORM_IDS[transform.upper()]
        out = (C.c_uint8 * (dst_cap + 64))()
        ol, ok = C.c_int32(0), C.c_int32(0)
        self._chk(self.L.knz_hip_transform_inverse_v(self.h, t, bs_version, data, len(data), out, dst_cap, C.byref(ol), C.byref(ok)))
        return ok.value, C.string_at(out, ol.value)

    def range_divide(self, d, r):
        """The RANGE decoder's divide on numpy uint64 arrays of (code - low, range) pairs: floor(d / r) as uint32."""
        import numpy as np
        d, r = np.ascontiguousarray(d, dtype=np.uint64), np.ascontiguousarray(r, dtype=np.uint64)
        q = np.zeros(len(d), dtype=np.uint32)
        self._chk(self.L.knz_hip_range_divide(self.h, d.ctypes.data, r.ctypes.data, len(d), q.ctypes.data))
        return q

    # ---- test hooks of csrc/prims.hpp, on device pointers (0 / None = absent)
    def prims_scan(self, op, d_in, d_out, n_max, d_n=None, d_total=None):
        """op 0: exclusive sum, 1: inclusive max, 2: inclusive min over min(n_max, *d_n) 32-bit words; d_in may equal d_out."""
        self._chk(self.L.knz_hip_prims_scan(self.h, op, C.c_void_p(d_in), C.c_void_p(d_out), n_max, C.c_void_p(d_n or None), C.c_void_p(d_total or None)))

    def prims_sort(self, key_bytes, has_val, keep, one_read, d_keys, d_vals, d_seg_base, n_seg, max_seg_len, lo_bit, hi_bit, d_keys_out, d_vals_out):
        """Stable sort of every segment on key bits [lo_bit, hi_bit) into d_keys_out / d_vals_out; raises when a guard byte around the
        sort's own buffers has changed."""
        self._chk(self.L.knz_hip_prims_sort(self.h, key_bytes, int(has_val), int(keep), int(one_read), C.c_void_p(d_keys), C.c_void_p(d_vals or None),
                                            C.c_void_p(d_seg_base), n_seg, max_seg_len, lo_bit, hi_bit, C.c_void_p(d_keys_out), C.c_void_p(d_vals_out or None)))

    # ---- profiling
    def set_profiling(self, on):
        self.L.knz_hip_set_profiling(self.h, 1 if on else 0)

    def kernel_times(self):
        arr = (KernelTime * 256)()
        n = self.L.knz_hip_get_kernel_times(self.h, arr, 256)
        return [(arr[i].name.decode(), arr[i].ms, arr[i].launches) for i in range(n)]


def prims_info():
    """(RS_TILE, RS_GROUP, SC_TILE, RS_MAXPASS) of csrc/prims.hpp: keys per radix tile, tiles per group of the column scan, words per scan
    tile, passes the one-read sort counts ahead. Needs no device."""
    out = (C.c_uint32 * 4)()
    rc = lib().knz_hip_prims_info(out)
    if rc != 0:
        raise KnzError(rc, "knz_hip_prims_info")
    return tuple(out)


def tpaq_params(stream_block_size, block_len, extra):
    """(states bytes, mixers, hash words, buffer bytes, contexts of the first and of the second SSE map) of the TPAQ (extra 0) / TPAQX
    (extra 1) predictor: the library's own restatement of the format's sizing, for tests. Needs no device."""
    out = (C.c_uint32 * 6)()
    rc = lib().knz_hip_tpaq_params(stream_block_size, block_len, extra, out)
    if rc != 0:
        raise KnzError(rc, "knz_hip_tpaq_params")
    return tuple(out)
