// C-ABI layer (include/knz_hip.h): context, workspaces, and the batch drivers that chain the
// transform / entropy / bit-assembly kernels on one HIP stream.
#include "common.hpp"
#include "stages.hpp"
#include "max_encoded.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <condition_variable>
#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace knz;

namespace knz {

const char* hipErrStr(hipError_t e) { return hipGetErrorString(e); }

struct WsBuf { void* p = nullptr; size_t cap = 0; };

struct ProfEntry { std::string name; hipEvent_t a, b; };

// A helper thread of a context that lives as long as the context (the parts of a BWT stage each need a host thread of their own:
// the suffix sort reads counters back between its rounds). Creating threads per call cost ~0.1 ms each on a 4-block batch.
struct Helper {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    bool has = false, done = true, quit = false;
    void loop()
    {
        for (;;) {
            std::function<void()> j;
            { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return has || quit; }); if (!has) return; j = std::move(job); has = false; }
            j();
            { std::lock_guard<std::mutex> l(m); done = true; }
            cv.notify_all();
        }
    }
    void run(std::function<void()> f)
    {
        if (!th.joinable()) th = std::thread(&Helper::loop, this);
        { std::lock_guard<std::mutex> l(m); job = std::move(f); has = true; done = false; }
        cv.notify_all();
    }
    void wait() { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return done; }); }
    void stop()
    {
        if (!th.joinable()) return;
        { std::lock_guard<std::mutex> l(m); quit = true; }
        cv.notify_all();
        th.join();
    }
};

struct Ctx {
    int device = 0;
    Helper helpers[3];
    hipStream_t stream = nullptr;
    bool ownStream = false;
    char err[512] = { 0 };
    std::map<std::string, WsBuf> ws;
    bool profiling = false;
    std::vector<ProfEntry> prof;
    void* pinned = nullptr;      // small pinned host scratch
    size_t pinnedCap = 0;
    std::recursive_mutex mu;     // a context is one stream + one set of workspaces: calls on it are serialised
    std::mutex errMu;            // the last-error string is also written by the copy entry points, which do not take `mu`
    // Copy engine beside the kernels: one stream per direction, outside the lock above, so that a host thread can move the next
    // batch in (or the last one out) while another thread sits in knz_hip_encode_blocks / knz_hip_decode_blocks.
    hipStream_t stream2[3] = { nullptr, nullptr, nullptr };       // side streams of fork_join (split BWT stages, decode lanes)
    hipEvent_t evFork = nullptr, evJoin[3] = { nullptr, nullptr, nullptr };
    std::mutex copyMu;
    hipStream_t copyIn = nullptr, copyOut = nullptr;
    std::vector<hipEvent_t> copyIdle;
    std::map<uint64_t, hipEvent_t> copyPending;
    uint64_t copyNext = 1;
    // knz_hip_copy_many's table on its way to the device: pinned, grown on demand, reused by the next call once tabStageEv (recorded
    // behind the upload) has passed
    void* tabStage = nullptr;
    size_t tabStageCap = 0;
    hipEvent_t tabStageEv = nullptr;
};
#define CTX_LOCK(c) std::lock_guard<std::recursive_mutex> ctx_lock_((c)->mu)

static int fail(Ctx* c, int code, const char* fmt, ...)
{
    std::lock_guard<std::mutex> el(c->errMu);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(c, -1, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// (s: the stream that uses the buffer first -- the KNZ_POISON_WS fill is queued there)
static int ws_get(Ctx* c, const std::string& name, size_t bytes, void** out, hipStream_t s)
{
    WsBuf& w = c->ws[name];
    if (w.cap < bytes) {
        if (w.p) HIPCHK(c, hipFree(w.p));
        w.p = nullptr; w.cap = 0;
        const size_t want = bytes + (bytes >> 3) + 4096;
        HIPCHK(c, hipMalloc(&w.p, want));
        w.cap = want;
    }
    *out = w.p;
    // KNZ_POISON_WS=1 (debugging aid): fill every workspace with a pattern on every request, so that a kernel that
    // relies on what an earlier call left behind fails deterministically instead of once in a few thousand runs
    static const int poison = getenv("KNZ_POISON_WS") ? atoi(getenv("KNZ_POISON_WS")) : 0;
    if (poison && bytes) HIPCHK(c, hipMemsetAsync(w.p, poison == 2 ? 0xFF : 0xA5, bytes, s));
    return 0;
}

// Lanes: lane -1 (a whole batch) and lane 0 use a workspace's plain name and the start of the pinned area. Lane k >= 1 -- part k of a split
// BWT / BWTS stage, or range k of a decode (the two never run at once and share) -- has workspaces of its own, named base + (k + 1), and
// slice k of the pinned area for its read-backs (the context's is 1 MiB).
static std::string lane_ws(const char* base, int lane) { return lane <= 0 ? std::string(base) : base + std::to_string(lane + 1); }
constexpr size_t PINNED_LANE_U32 = 32768;
static u32* lane_pinned(Ctx* c, int lane) { return reinterpret_cast<u32*>(c->pinned) + PINNED_LANE_U32 * (lane < 0 ? 0 : lane); }

// The fixed host words of the batch drivers (Encoder, Decoder) in the same area, all at the start of lane 0's slice:
//   byte 0      total      the encoder's read-back of the output's size (bits of one stream, bytes of many)
//   byte 8      marked     the blocks that did not fit a two-tier coder's first staging, read back with the total
//   byte 0      walk       the decoder's read-back of the block walk (a call encodes or decodes, and the context is locked)
//   byte 4096   hostedSum  a hosted block's checksum on its way to the device
//   byte 0 ...  caps       the encoder's two capacity arrays of nBlocks words each on their way to the device, over as much of the
//                          area as they need, all lanes' slices included
// The capacity arrays are uploaded before the first stage runs, and the encoder synchronises its stream behind the upload
// (Encoder::capacities): they are gone before a stage reads anything back into a lane's slice and before total and marked are
// written. A hosted call has one block, so its capacities (bytes 0-7) stay clear of hostedSum, which is uploaded in front of them.
// The stages synchronise behind their own read-backs; total, marked and walk are read behind a synchronisation of the context's
// stream, at points where no stage runs.
struct WalkResultHost { u64 endBit; int64_t nBlocks; int32_t ended; int32_t error; };
struct PinnedWords {
    u8* base;
    explicit PinnedWords(Ctx* c) : base(static_cast<u8*>(c->pinned)) {}
    u64* total() const { return reinterpret_cast<u64*>(base); }
    u32* marked() const { return reinterpret_cast<u32*>(base + 8); }
    WalkResultHost* walk() const { return reinterpret_cast<WalkResultHost*>(base); }
    u64* hostedSum() const { return reinterpret_cast<u64*>(base + 4096); }
    u32* caps() const { return reinterpret_cast<u32*>(base); }
};

thread_local ProfHook* g_prof = nullptr;

struct CtxProf : ProfHook {
    Ctx* c; int idx = -1;
    explicit CtxProf(Ctx* ctx) : c(ctx) {}
    void begin(const char* name) override {
        ProfEntry e; e.name = name;
        hipEventCreate(&e.a); hipEventCreate(&e.b);
        hipEventRecord(e.a, c->stream);
        c->prof.push_back(e);
        idx = (int)c->prof.size() - 1;
    }
    void end() override { if (idx >= 0) hipEventRecord(c->prof[idx].b, c->stream); idx = -1; }
};

// Installs the hook for the duration of one API call when profiling is enabled.
struct ProfInstall {
    CtxProf hook;
    explicit ProfInstall(Ctx* c) : hook(c) { g_prof = c->profiling ? &hook : nullptr; }
    ~ProfInstall() { g_prof = nullptr; }
};

// memset / memcpy segments are timed under their own names
struct ProfScope {
    bool on;
    ProfScope(Ctx*, const char* name) : on(g_prof != nullptr) { if (on) g_prof->begin(name); }
    ~ProfScope() { if (on) g_prof->end(); }
};

static int count_transforms(uint64_t t, int* tok)
{
    int nb = 0;
    for (int i = 0; i < 8; i++) {
        const int v = (int)((t >> (42 - 6 * i)) & 63);
        if (v != 0 || i == 0) tok[nb++] = v;
    }
    return nb;
}

static bool host_stage_id(int t) { return t == KNZ_T_TEXT || t == KNZ_T_UTF; }

}  // namespace knz

extern "C" {

int knz_hip_device_count(int* count)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = (e == hipSuccess) ? n : 0;
    return e == hipSuccess ? 0 : -1;
}

int knz_hip_create(int device, void* stream, knz_ctx** out)
{
    *out = nullptr;
    Ctx* c = new Ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return -1; }
    if (stream) { c->stream = (hipStream_t)stream; c->ownStream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return -1; }
        c->ownStream = true;
    }
    c->pinnedCap = 1 << 20;
    if (hipHostMalloc(&c->pinned, c->pinnedCap, hipHostMallocDefault) != hipSuccess) { delete c; return -1; }
    *out = reinterpret_cast<knz_ctx*>(c);
    return 0;
}

void knz_hip_destroy(knz_ctx* ctx)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return;
    for (Helper& h : c->helpers) h.stop();
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    for (auto& kv : c->ws) if (kv.second.p) hipFree(kv.second.p);
    for (auto& e : c->prof) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    if (c->pinned) hipHostFree(c->pinned);
    if (c->tabStage) hipHostFree(c->tabStage);
    if (c->tabStageEv) hipEventDestroy(c->tabStageEv);
    for (auto& kv : c->copyPending) { hipEventSynchronize(kv.second); hipEventDestroy(kv.second); }
    for (auto& e : c->copyIdle) hipEventDestroy(e);
    for (int k = 0; k < 3; k++) { if (c->stream2[k]) hipStreamDestroy(c->stream2[k]); if (c->evJoin[k]) hipEventDestroy(c->evJoin[k]); }
    if (c->evFork) hipEventDestroy(c->evFork);
    if (c->copyIn) hipStreamDestroy(c->copyIn);
    if (c->copyOut) hipStreamDestroy(c->copyOut);
    if (c->ownStream) hipStreamDestroy(c->stream);
    delete c;
}

static std::atomic<int>& bwt_split_knob()
{
    static std::atomic<int> v([] { const char* e = getenv("KNZ_BWT_SPLIT"); const int x = e ? atoi(e) : 3; return x < 1 ? 1 : (x > 4 ? 4 : x); }());
    return v;
}

// fewest blocks a part of a split BWT stage may have (KNZ_BWT_PART_MIN / knob "bwt_part_min"; see bwt_parts_wanted)
static std::atomic<int>& bwt_part_min_knob()
{
    static std::atomic<int> v([] { const char* e = getenv("KNZ_BWT_PART_MIN"); const int x = e ? atoi(e) : 2; return x < 1 ? 1 : x; }());
    return v;
}

// ranges of a batch that knz_hip_decode_blocks runs side by side on streams of their own (KNZ_DEC_PARTS / knob "dec_parts"; Decoder::plan)
static std::atomic<int>& dec_parts_knob()
{
    static std::atomic<int> v([] { const char* e = getenv("KNZ_DEC_PARTS"); const int x = e ? atoi(e) : 3; return x < 1 ? 1 : (x > 3 ? 3 : x); }());
    return v;
}

// fewest blocks such a range may have (KNZ_DEC_PART_MIN)
static std::atomic<int>& dec_part_min_knob()
{
    static std::atomic<int> v([] { const char* e = getenv("KNZ_DEC_PART_MIN"); const int x = e ? atoi(e) : 2; return x < 1 ? 1 : x; }());
    return v;
}

int knz_hip_tune(const char* name, int value)
{
    if (name == nullptr) return -1;
    if (!strcmp(name, "dec_parts")) { dec_parts_knob().store(value < 1 ? 1 : (value > 3 ? 3 : value)); return 0; }
    if (!strcmp(name, "bwt_part_min")) { bwt_part_min_knob().store(value < 1 ? 1 : value); return 0; }
    if (!strcmp(name, "mtf_tile")) return mtft_tune(value);
    if (!strcmp(name, "mtf_chain")) return mtft_tune_chain(value);
    if (!strcmp(name, "lz_serial_decode")) { lz_serial_decode(value ? 1 : 0); return 0; }
    if (!strcmp(name, "bwt_split")) { bwt_split_knob().store(value < 1 ? 1 : (value > 4 ? 4 : value)); return 0; }
    if (!strcmp(name, "bwt_inv_jump_all")) return bwt_inverse_tune(0, value);
    if (!strcmp(name, "bwt_inv_ruler_log")) return bwt_inverse_tune(1, value);
    if (!strcmp(name, "bwt_inv_wide")) return bwt_inverse_tune(2, value);
    return bwt_forward_tune(name, value);
}

// (a copy taken under the lock the writers hold, into a buffer of the calling thread: lane contexts are shared between the stream
// classes' worker threads and the copy entry points run outside `mu`, so the context's own buffer may be rewritten while it is read)
const char* knz_hip_last_error(knz_ctx* ctx)
{
    if (!ctx) return "null context";
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    thread_local char copy[sizeof(c->err)];
    std::lock_guard<std::mutex> el(c->errMu);
    memcpy(copy, c->err, sizeof(copy));
    copy[sizeof(copy) - 1] = 0;
    return copy;
}

int knz_hip_set_profiling(knz_ctx* ctx, int enabled)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    c->profiling = enabled != 0;
    for (auto& e : c->prof) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    c->prof.clear();
    return 0;
}

int knz_hip_get_kernel_times(knz_ctx* ctx, knz_kernel_time* out, int cap)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    hipStreamSynchronize(c->stream);
    std::vector<std::string> order;
    std::map<std::string, std::pair<float, uint64_t>> agg;
    for (auto& e : c->prof) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) ms = 0;
        if (!agg.count(e.name)) order.push_back(e.name);
        agg[e.name].first += ms;
        agg[e.name].second += 1;
    }
    int n = 0;
    for (auto& nm : order) {
        if (n >= cap) break;
        memset(&out[n], 0, sizeof(out[n]));
        snprintf(out[n].name, sizeof(out[n].name), "%s", nm.c_str());
        out[n].ms = agg[nm].first;
        out[n].launches = agg[nm].second;
        n++;
    }
    for (auto& e : c->prof) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    c->prof.clear();
    return n;
}

int knz_hip_malloc(knz_ctx* ctx, size_t bytes, void** d_ptr)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc(d_ptr, bytes ? bytes : 1));
    return 0;
}

int knz_hip_free(knz_ctx* ctx, void* d_ptr)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    HIPCHK(c, hipFree(d_ptr));
    return 0;
}

int knz_hip_memcpy_h2d(knz_ctx* ctx, void* d_dst, const void* src, size_t bytes)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    HIPCHK(c, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int knz_hip_memcpy_d2h(knz_ctx* ctx, void* dst, const void* d_src, size_t bytes)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    HIPCHK(c, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int copy_async(Ctx* c, void* dst, const void* src, size_t bytes, bool in, uint64_t* ticket)
{
    *ticket = 0;
    std::lock_guard<std::mutex> l(c->copyMu);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t& st = in ? c->copyIn : c->copyOut;
    if (st == nullptr) HIPCHK(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipEvent_t ev;
    if (!c->copyIdle.empty()) { ev = c->copyIdle.back(); c->copyIdle.pop_back(); }
    else HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = bytes ? hipMemcpyAsync(dst, src, bytes, in ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st) : hipSuccess;
    if (e == hipSuccess) e = hipEventRecord(ev, st);
    if (e != hipSuccess) {                                       // the event goes back to the idle list, the caller gets no ticket
        c->copyIdle.push_back(ev);
        return fail(c, -1, "asynchronous copy failed: %s", hipGetErrorString(e));
    }
    *ticket = c->copyNext++;
    c->copyPending[*ticket] = ev;
    return 0;
}

int knz_hip_memcpy_h2d_async(knz_ctx* ctx, void* d_dst, const void* src, size_t bytes, uint64_t* ticket)
{
    return copy_async(reinterpret_cast<Ctx*>(ctx), d_dst, src, bytes, true, ticket);
}

int knz_hip_memcpy_d2h_async(knz_ctx* ctx, void* dst, const void* d_src, size_t bytes, uint64_t* ticket)
{
    return copy_async(reinterpret_cast<Ctx*>(ctx), dst, d_src, bytes, false, ticket);
}

int knz_hip_copy_wait(knz_ctx* ctx, uint64_t ticket)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipEvent_t ev;
    {
        std::lock_guard<std::mutex> l(c->copyMu);
        auto it = c->copyPending.find(ticket);
        if (it == c->copyPending.end()) return 0;               // unknown or already waited for
        ev = it->second;
        c->copyPending.erase(it);
    }
    const hipError_t e = hipEventSynchronize(ev);
    {
        std::lock_guard<std::mutex> l(c->copyMu);
        c->copyIdle.push_back(ev);
    }
    if (e != hipSuccess) return fail(c, -1, "copy failed: %s", hipGetErrorString(e));
    return 0;
}

int knz_hip_host_alloc(size_t bytes, void** ptr)
{
    *ptr = nullptr;
    return hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? 0 : -1;
}

int knz_hip_host_free(void* ptr) { return (ptr == nullptr || hipHostFree(ptr) == hipSuccess) ? 0 : -1; }

int knz_hip_sync(knz_ctx* ctx)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int knz_hip_shift_bits(knz_ctx* ctx, const uint8_t* d_in, uint64_t nbits, uint32_t r, uint8_t* d_out)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (c == nullptr || d_in == nullptr || d_out == nullptr || r == 0 || r > 7) return KNZ_ERR_INVALID_PARAM;
    CTX_LOCK(c);
    HIPCHK(c, hipSetDevice(c->device));
    launch_shift_bits(c->stream, d_in, nbits, r, d_out);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// shared plumbing
// ------------------------------------------------------------------------------------------------
struct SeqWs {
    SeqArrays a;
    u32* d_capEven; u32* d_capOdd;
    const u8** d_viewPtr;
    u8** d_entDst;
    u8* A; u8* B; u64 S;
    u32* scratch;
};

// (the workspaces of `lane`, first used on stream s)
static int seq_alloc(Ctx* c, int nBlocks, u64 S, bool needAB, size_t scratchU32, SeqWs* w, int lane, hipStream_t s)
{
    u8* base;
    const size_t nb = (size_t)nBlocks;
    // one slab for all small per-block arrays
    const size_t bytes = nb * (6 * 1 + 4 * 6 + 8 * 4) + 1024;
    if (int r = ws_get(c, lane_ws("seqSmall", lane), bytes + 256, (void**)&base, s)) return r;
    size_t off = 0;
    auto take = [&](size_t sz, size_t align) { off = (off + align - 1) & ~(align - 1); u8* p = base + off; off += sz; return p; };
    w->a.src = (const u8**)take(nb * 8, 16);
    w->a.dst = (u8**)take(nb * 8, 16);
    w->d_viewPtr = (const u8**)take(nb * 8, 16);
    w->d_entDst = (u8**)take(nb * 8, 16);
    w->a.len = (u32*)take(nb * 4, 16);
    w->a.alen = (u32*)take(nb * 4, 16);
    w->a.cap = (u32*)take(nb * 4, 16);
    w->a.newLen = (u32*)take(nb * 4, 16);
    w->d_capEven = (u32*)take(nb * 4, 16);
    w->d_capOdd = (u32*)take(nb * 4, 16);
    w->a.where = take(nb, 16);
    w->a.swaps = take(nb, 16);
    w->a.active = take(nb, 16);
    w->a.skip = take(nb, 16);
    w->a.ok = take(nb, 16);
    w->a.dtype = take(nb, 16);
    w->a.bufCap = w->d_capEven;
    w->a.dataCap = w->d_capOdd;
    w->S = S;
    w->A = w->B = nullptr;
    if (needAB) {
        if (int r = ws_get(c, lane_ws("xfA", lane), (size_t)S * nb + 256, (void**)&w->A, s)) return r;
        if (int r = ws_get(c, lane_ws("xfB", lane), (size_t)S * nb + 256, (void**)&w->B, s)) return r;
    }
    w->scratch = nullptr;
    if (scratchU32) { if (int r = ws_get(c, lane_ws("xfScratch", lane), scratchU32 * 4 + 64, (void**)&w->scratch, s)) return r; }
    return 0;
}

// The stage record of a batch over the workspaces `w` (bsVersion, maxCap and dtype are left to the caller)
static XfStage xf_stage(const SeqWs& w, int nBlocks, u32 maxLen, int entropyType)
{
    XfStage st;
    st.src = w.a.src; st.dst = w.a.dst; st.len = w.a.alen; st.cap = w.a.cap; st.ok = w.a.ok; st.newLen = w.a.newLen;
    st.nBlocks = nBlocks; st.maxLen = maxLen; st.scratchU32 = w.scratch; st.entropyType = entropyType;
    return st;
}

// ------------------------------------------------------------------------------------------------
// the device transforms
// ------------------------------------------------------------------------------------------------
// One launch of a stage: on stream s over st, with the stage's own scratch (ws, wsBytes) and a pinned read-back area. Returns 0, or a
// failure code with the context's error set.
struct StageCall { Ctx* c; hipStream_t s; const XfStage& st; void* ws; size_t wsBytes; u32* pinned; };

static int failed(const StageCall& k, const char* what) { return fail(k.c, -1, "%s failed: %s", what, hipGetErrorString(hipGetLastError())); }

// Whether a stage over a whole batch may run as several parts side by side (bwt_parts_wanted), and whether each part needs a host thread
// of its own (a stage that reads the device back between its launches)
enum Split { NO_SPLIT, SPLIT_QUEUED, SPLIT_THREADS };

struct XfDir {
    size_t (*scratchU32)(int nBlocks, u32 maxLen);   // words of the chain's shared stage scratch (XfStage::scratchU32), or nullptr
    size_t (*wsBytes)(int nBlocks, u32 maxLen);      // bytes of the stage's own scratch XfInfo::ws, or nullptr
    size_t (*wsBytesOf)(const XfStage&);             // the same for a stage whose scratch depends on more of the stage record (TEXT)
    int (*launch)(const StageCall&);
    Split split;
};

// What the drivers know of one device transform. Everything else about it lives in its launchers, and its size bound in max_encoded.hpp.
struct XfInfo {
    int id;
    const char* ws;              // name of the stage's own scratch (one name for both directions; stages that never run at once share one)
    XfDir fwd, inv;
    bool setsType = false;       // reads and sets the per-block data type (XfStage::dtype)
    bool ignoresType = false;    // would have to read the data type and does not: refused behind a stage that sets it
    bool lanes = true;           // the inverse may run in decode lanes (Decoder::plan)
};

static int lz_inverse(const StageCall& k)
{
    Ctx* c = k.c; const XfStage& st = k.st;
    void* sc = nullptr;
    size_t bytes = 0;
    if (st.maxCap != 0 && st.maxCap <= (1u << 30) && !lz_serial_decode(-1)) {
        // about 20 bytes per output byte; when the device cannot spare that (1 GiB blocks, a 2 GiB batch), or the workspace would
        // exceed the budget below, the blocks are decoded by the one-wave-per-block decoder, which needs no scratch
        bytes = lz_inverse_scratch_bytes(st.nBlocks, st.maxCap);
        static const size_t budget = getenv("KNZ_LZ_INV_SCRATCH_MAX") ? (size_t)atoll(getenv("KNZ_LZ_INV_SCRATCH_MAX")) : ((size_t)48 << 30);
        WsBuf& wb = c->ws["lzInvScratch"];
        if (bytes > budget) { bytes = 0; }
        else if (wb.cap >= bytes) sc = wb.p;
        else {
            if (wb.p) { HIPCHK(c, hipFree(wb.p)); wb.p = nullptr; wb.cap = 0; }
            const size_t want = bytes + (bytes >> 3) + 4096;
            void* p = nullptr;
            if (hipMalloc(&p, want) == hipSuccess) { wb.p = p; wb.cap = want; sc = p; }
            else { (void)hipGetLastError(); bytes = 0; }           // out of memory: the serial decoder
        }
    }
    launch_lz_inverse(k.s, st, sc, bytes, st.maxCap);
    return 0;
}

static const XfInfo XF[] = {
    { .id = KNZ_T_ZRLT, .fwd = { .scratchU32 = zrlt_scratch_u32, .launch = [](const StageCall& k) { launch_zrlt_forward(k.s, k.st); return 0; } },
                        .inv = { .scratchU32 = zrlt_scratch_u32, .launch = [](const StageCall& k) { launch_zrlt_inverse(k.s, k.st); return 0; } } },
    { .id = KNZ_T_MTFT, .fwd = { .scratchU32 = mtft_scratch_u32, .launch = [](const StageCall& k) { launch_mtft_forward(k.s, k.st); return 0; } },
                        .inv = { .scratchU32 = mtft_scratch_u32, .launch = [](const StageCall& k) { launch_mtft_inverse(k.s, k.st); return 0; } } },
    // (the BWT and BWTS stages synchronise their stream: the suffix sort reads counters back between rounds, the BWTS inverse reads
    // convergence flags every round; the BWT inverse only queues launches)
    { .id = KNZ_T_BWT, .ws = "bwtScratch",
      .fwd = { .wsBytes = [](int nb, u32 m) { return bwt_forward_scratch_bytes(nb, m, (size_t)nb * m); },
               .launch = [](const StageCall& k) { return launch_bwt_forward(k.s, k.st, k.ws, k.wsBytes, k.pinned) ? failed(k, "BWT forward") : 0; },
               .split = SPLIT_THREADS },
      .inv = { .wsBytes = [](int nb, u32 m) { return bwt_inverse_scratch_bytes(nb, m, (size_t)nb * m); },
               .launch = [](const StageCall& k) { return launch_bwt_inverse(k.s, k.st, k.ws, k.wsBytes, k.pinned) ? failed(k, "BWT inverse") : 0; },
               .split = SPLIT_QUEUED } },
    { .id = KNZ_T_BWTS, .ws = "bwtScratch",
      .fwd = { .wsBytes = [](int nb, u32 m) { return bwts_forward_scratch_bytes(nb, m, (size_t)nb * m); },
               .launch = [](const StageCall& k) { return launch_bwts_forward(k.s, k.st, k.ws, k.wsBytes, k.pinned) ? failed(k, "BWTS forward") : 0; },
               .split = SPLIT_THREADS },
      .inv = { .wsBytes = [](int nb, u32 m) { return bwts_inverse_scratch_bytes(nb, m, (size_t)nb * m); },
               .launch = [](const StageCall& k) { return launch_bwts_inverse(k.s, k.st, k.ws, k.wsBytes, k.pinned) ? failed(k, "BWTS inverse") : 0; },
               .split = SPLIT_THREADS } },
    { .id = KNZ_T_SRT, .fwd = { .scratchU32 = srt_scratch_u32, .launch = [](const StageCall& k) { launch_srt_forward(k.s, k.st); return 0; } },
                       .inv = { .scratchU32 = srt_inverse_scratch_u32, .launch = [](const StageCall& k) { launch_srt_inverse(k.s, k.st); return 0; } } },
    { .id = KNZ_T_RLT, .fwd = { .launch = [](const StageCall& k) { launch_rlt_forward(k.s, k.st); return 0; } },
                       .inv = { .launch = [](const StageCall& k) { launch_rlt_inverse(k.s, k.st); return 0; } } },
    // LZ / LZX behind PACK would have to take PACK's data type (min match 6 for DNA, refusal of SMALL_ALPHABET, LZCodec.cpp:179-191);
    // the device LZ stages do not read it yet, so such chains are refused rather than encoded differently from the reference. The
    // inverse has one scratch (lzInvScratch, lz_inverse), so it runs on no decode lane.
    { .id = KNZ_T_LZ, .ws = "lzScratch",
      .fwd = { .wsBytes = [](int nb, u32 m) { return lz_forward_scratch_bytes(KNZ_T_LZ, nb, m); },
               .launch = [](const StageCall& k) { return launch_lz_forward(k.s, k.st, KNZ_T_LZ, k.ws, k.wsBytes) ? failed(k, "LZ forward") : 0; } },
      .inv = { .launch = lz_inverse },
      .ignoresType = true, .lanes = false },
    { .id = KNZ_T_LZX, .ws = "lzScratch",
      .fwd = { .wsBytes = [](int nb, u32 m) { return lz_forward_scratch_bytes(KNZ_T_LZX, nb, m); },
               .launch = [](const StageCall& k) { return launch_lz_forward(k.s, k.st, KNZ_T_LZX, k.ws, k.wsBytes) ? failed(k, "LZ forward") : 0; } },
      .inv = { .launch = lz_inverse },
      .ignoresType = true, .lanes = false },
    { .id = KNZ_T_RANK, .fwd = { .launch = [](const StageCall& k) { launch_sbrt_forward(k.s, k.st, 2); return 0; } },
                        .inv = { .launch = [](const StageCall& k) { launch_sbrt_inverse(k.s, k.st, 2); return 0; } } },
    { .id = KNZ_T_TIMESTAMP, .fwd = { .launch = [](const StageCall& k) { launch_sbrt_forward(k.s, k.st, 3); return 0; } },
                             .inv = { .launch = [](const StageCall& k) { launch_sbrt_inverse(k.s, k.st, 3); return 0; } } },
    // (AliasCodec; the data type it starts from is preset from the block's magic or taken from the host stages, Encoder::data_types)
    { .id = KNZ_T_PACK, .ws = "packScratch",
      .fwd = { .wsBytes = pack_scratch_bytes, .launch = [](const StageCall& k) { launch_pack_forward(k.s, k.st, k.ws); return 0; } },
      .inv = { .wsBytes = pack_scratch_bytes, .launch = [](const StageCall& k) { launch_pack_inverse(k.s, k.st, k.ws); return 0; } },
      .setsType = true },
    // (DNA, id 19: AliasCodec with the Context entry packOnlyDNA, TransformFactory.hpp:293-294. PACK's launchers; the forward refuses a
    // preset type other than UNDEFINED or DNA and a block whose detection does not say DNA, after it wrote what detection found. The
    // inverse is PACK's. The Context entry outlives the stage: a PACK behind DNA in one chain is built with it too, Encoder::transforms)
    { .id = KNZ_T_DNA, .ws = "packScratch",
      .fwd = { .wsBytes = pack_scratch_bytes, .launch = [](const StageCall& k) { XfStage st = k.st; st.onlyDNA = 1; launch_pack_forward(k.s, st, k.ws); return 0; } },
      .inv = { .wsBytes = pack_scratch_bytes, .launch = [](const StageCall& k) { launch_pack_inverse(k.s, k.st, k.ws); return 0; } },
      .setsType = true },
    // (FSDCodec; it leaves MULTIMEDIA or detectSimpleType's verdict on the blocks it looks at, which RLT behind it reads)
    { .id = KNZ_T_MM, .ws = "mmScratch",
      .fwd = { .wsBytes = mm_scratch_bytes, .launch = [](const StageCall& k) { launch_mm_forward(k.s, k.st, k.ws); return 0; } },
      .inv = { .wsBytes = mm_scratch_bytes, .launch = [](const StageCall& k) { launch_mm_inverse(k.s, k.st, k.ws); return 0; } },
      .setsType = true },
    // (LZPCodec; it neither reads nor writes the data type. Both directions keep a table per block in the stage's scratch, which
    // run_stage takes per lane through lane_ws, so the inverse runs in decode lanes, each lane with tables of its own)
    { .id = KNZ_T_LZP, .ws = "lzpScratch",
      .fwd = { .wsBytes = lzp_scratch_bytes, .launch = [](const StageCall& k) { launch_lzp_forward(k.s, k.st, k.ws); return 0; } },
      .inv = { .wsBytes = lzp_scratch_bytes, .launch = [](const StageCall& k) { launch_lzp_inverse(k.s, k.st, k.ws); return 0; } } },
    // (UTFCodec; it reads the data type -- preset from the block's magic, or what TEXT left on the host, Encoder::data_types -- and writes UTF8,
    // which LZ and LZX treat like UNDEFINED (LZCodec.cpp:182-191). The refusal of LZ / LZX behind a stage that sets the type is kept for
    // UTF all the same: a block UTF refuses keeps its preset type, which the device LZ stages do not read. Scratch per lane like LZP's, so
    // the inverse runs in decode lanes. Behind the hosted prefix (TEXT) it is a device stage like any other, parse_chain)
    { .id = KNZ_T_UTF, .ws = "utfScratch",
      .fwd = { .wsBytes = utf_scratch_bytes, .launch = [](const StageCall& k) { launch_utf_forward(k.s, k.st, k.ws); return 0; } },
      .inv = { .wsBytes = utf_scratch_bytes, .launch = [](const StageCall& k) { launch_utf_inverse(k.s, k.st, k.ws); return 0; } },
      .setsType = true },
    // (ROLZCodec2; it reads the data type -- EXE and DNA change its key and its minimum match -- and writes detectSimpleType's verdict
    // where it found none, which RLT behind it reads. About 8.3 MiB of tables per block that runs at once, per lane like LZP's, so the
    // inverse runs in decode lanes. ROLZ proper, id 11, codes its streams with ANS coders of its own and has no kernel)
    { .id = KNZ_T_ROLZX, .ws = "rolzxScratch",
      .fwd = { .wsBytes = rolzx_scratch_bytes, .launch = [](const StageCall& k) { launch_rolzx_forward(k.s, k.st, k.ws); return 0; } },
      .inv = { .wsBytes = rolzx_scratch_bytes, .launch = [](const StageCall& k) { launch_rolzx_inverse(k.s, k.st, k.ws); return 0; } },
      .setsType = true },
    // (EXECodec; it reads the data type -- preset from the block's magic: ELF, PE and Mach-O blocks come as EXE -- and writes EXE on a
    // block it rewrites, or what its detection found on a block that detection rejects: ROLZX behind it keys EXE blocks 3 bytes back,
    // PACK behind it refuses them. Scratch per lane like LZP's, so the inverse runs in decode lanes. Its verdict on the way back
    // depends on the capacity, so the last inverse stage of a stream judges by XfStage::capModel as UTF does)
    { .id = KNZ_T_EXE, .ws = "exeScratch",
      .fwd = { .wsBytes = exe_scratch_bytes, .launch = [](const StageCall& k) { launch_exe_forward(k.s, k.st, k.ws); return 0; } },
      .inv = { .wsBytes = exe_scratch_bytes, .launch = [](const StageCall& k) { launch_exe_inverse(k.s, k.st, k.ws); return 0; } },
      .setsType = true },
    // (TextCodec, in the encoding the stream's entropy coder asks for; it reads the data type -- UNDEFINED, TEXT and BIN blocks are looked
    // at -- and writes TEXT, or the type its statistics found on a block that is no text, which UTF, PACK and ROLZX behind it read. Its
    // hash map is sized by the stream's block size (XfStage::blockSize), so its scratch is; per lane like LZP's, so the inverse runs in
    // decode lanes, and the last inverse stage of a stream judges by XfStage::capModel as UTF does. In front of a chain it may still run
    // on the host: knz_hip_encode_block_hosted)
    { .id = KNZ_T_TEXT, .ws = "textScratch",
      .fwd = { .wsBytesOf = [](const XfStage& st) { return text_scratch_bytes(st.nBlocks, st.maxLen, st.blockSize); },
               .launch = [](const StageCall& k) { launch_text_forward(k.s, k.st, k.ws); return 0; } },
      .inv = { .wsBytesOf = [](const XfStage& st) { return text_scratch_bytes(st.nBlocks, st.maxLen, st.blockSize); },
               .launch = [](const StageCall& k) { launch_text_inverse(k.s, k.st, k.ws); return 0; } },
      .setsType = true },
};

static const XfInfo* xf_info(int t) { for (const XfInfo& x : XF) if (x.id == t) return &x; return nullptr; }

static int unsupported(Ctx* c, int t) { return fail(c, KNZ_ERR_INVALID_CODEC, "transform id %d not implemented on device", t); }

static size_t scratch_u32(const XfDir& d, int nBlocks, u32 maxLen) { return d.scratchU32 ? d.scratchU32(nBlocks, maxLen) : 0; }

// ------------------------------------------------------------------------------------------------
// the device entropy coders
// ------------------------------------------------------------------------------------------------
// One batch for an encoder: the blocks behind the transforms (view), their ChunkDesc slots (block b owns maxChunks = chunksPerBlock *
// slots per chunk of the nSlots at desc), and what the coders that write copy blocks themselves go by (origLen, copyThreshold).
// rbsz is the "blockSize" of the stream's Context (per-stage calls pass it) and extra the row's, both TPAQ's.
struct EcEnc {
    Ctx* c; hipStream_t s; BlockView view; const u32* origLen; u32 copyThreshold; int nBlocks; u64 S;
    int chunksPerBlock, maxChunks; size_t nSlots; ChunkDesc* desc; u32 rbsz; int extra;
};

// What an encoder leaves for the framing and for a second tier: the header base and stride launch_assemble reads, the device word that
// counts the blocks which did not fit their staging (two-tier coders), TPAQ's tables
struct EcStaged { u8* hdr = nullptr; u32 hdrStride = TMP_STRIDE; u32* marked = nullptr; void* tables = nullptr; };

// One range of blocks for a decoder, on stream s with the workspaces of `lane` (lane_ws). maxChunks and nSlots count ENT_CHUNK chunks.
struct EcDec {
    Ctx* c; hipStream_t s; int lane; BitSrc src; DecBlock* blk; int nb; u64 S; int maxChunks; size_t nSlots;
    int framing, bsVersion; u32 rbsz; int extra; u8* const* dst;
};

// What the drivers know of one entropy coder. Everything else about it lives in its launchers.
struct EcInfo {
    int id;
    u32 entChunk;                // chunk length of the framing's arithmetic (launch_block_sum, launch_assemble)
    u32 slots = 1;               // ChunkDesc slots per chunk, or
    int (*slotsOf)(u64 S) = nullptr;                       // the same where it depends on the longest block
    bool twoTier = false;        // bound() is a first tier: the coders behind BinaryEntropyEncoder (binary_coder.hpp)
    int extra = 0;               // TPAQ / TPAQX
    size_t (*bound)(size_t n, size_t nb) = nullptr;        // the row's term of knz_hip_encode_bound; nullptr: default_bound
    int (*encode)(const EcEnc&, EcStaged*);                // takes the coder's workspaces and launches
    int (*again)(const EcEnc&, const EcStaged&, CmBigAlloc, void* user) = nullptr;      // launch_cm_encode_again's contract (stages.hpp)
    int (*decode)(const EcDec&);
};

// worst case: every symbol emits 16 bits (ANS) or 12 bits (Huffman) plus per-chunk headers
static size_t default_bound(size_t n, size_t nb) { return 2 * n + nb * 64 + ((n / ENT_CHUNK) + nb) * (HDR_BYTES + 32) + 4096; }

// CM: no bound is proved below the format's 32 bytes per byte, so this is the FIRST tier, what the encoder stages a block at
// (n + n / 8, cm.hip) plus var-ints and tails. An encode whose stream is longer fails with KNZ_ERR_WRITE_FILE and names the size;
// 32 * n on top of this value always holds it (include/knz_hip.h).
// (TPAQ and TPAQX: the same coder behind another predictor, the same two tiers)
static size_t binary_bound(size_t n, size_t nb) { return (cm_tier1_div() ? n / cm_tier1_div() : n + n / 8) + nb * 64 + nb * (size_t)CM_MAX_CHUNKS * 16 + 4096; }

static int ans1_encode(const EcEnc& k, EcStaged* o)
{
    const size_t nCh = (size_t)k.nBlocks * k.chunksPerBlock;
    Ans1EncWs aw;
    aw.payStride = (2ull * std::min<u64>(k.S, ANS1_CHUNK) + 511) & ~255ull;
    if (int r = ws_get(k.c, "ans1Hist", ans1_hist_bytes(nCh), (void**)&aw.hist, k.s)) return r;
    if (int r = ws_get(k.c, "ans1EncTab", ans1_enctab_bytes(nCh), (void**)&aw.encTab, k.s)) return r;
    if (int r = ws_get(k.c, "chunkTmp", (size_t)HDR_BYTES * k.nSlots, (void**)&aw.hdr, k.s)) return r;
    if (int r = ws_get(k.c, "ans1Pay", (size_t)aw.payStride * nCh, (void**)&aw.pay, k.s)) return r;
    o->hdr = aw.hdr;
    o->hdrStride = HDR_BYTES;
    launch_ans1_encode(k.s, k.view, k.nBlocks, k.chunksPerBlock, k.desc, aw);
    return 0;
}

// (its metadata by its own 4 MiB chunks, not by the ENT_CHUNK slots)
static int ans1_decode(const EcDec& k)
{
    const int chunksPerBlock = (int)((k.S + ANS1_CHUNK - 1) / ANS1_CHUNK);
    const size_t nCh = (size_t)k.nb * chunksPerBlock;
    Ans1DecWs aw;
    if (int r = ws_get(k.c, lane_ws("ans1Meta", k.lane), ans1_meta_bytes(nCh), &aw.meta, k.s)) return r;
    if (int r = ws_get(k.c, lane_ws("ans1SlotTab", k.lane), ans1_slottab_bytes(nCh), (void**)&aw.slotTab, k.s)) return r;
    launch_ans1_decode(k.s, k.src, k.blk, k.nb, chunksPerBlock, aw, k.dst);
    return 0;
}

static int fpaq_encode(const EcEnc& k, EcStaged* o)
{
    const u64 fStride = (4u << 20) + (4u << 17) + 256;      // FPAQEncoder.cpp:65-68 buffer size (+ slack)
    u16* d_fprobs;
    if (int r = ws_get(k.c, "chunkTmp", (size_t)fStride * k.nSlots, (void**)&o->hdr, k.s)) return r;
    if (int r = ws_get(k.c, "fpaqProbs", fpaq_probs_bytes(k.nBlocks, k.S), (void**)&d_fprobs, k.s)) return r;
    launch_fpaq_encode(k.s, k.view, k.origLen, k.copyThreshold, k.nBlocks, k.maxChunks, k.desc, o->hdr, fStride, d_fprobs, k.S);
    return 0;
}

// The staging the binary coders share: block b at hdr + b * cm_stage_stride(S), and the control words, of which the first counts the
// blocks that did not fit (read back with the total; they are coded again into 32 n + 16 bytes each, workspace taken only then)
static int binary_staging(const EcEnc& k, EcStaged* o)
{
    if (int r = ws_get(k.c, "chunkTmp", (size_t)cm_stage_stride(k.S) * k.nBlocks, (void**)&o->hdr, k.s)) return r;
    return ws_get(k.c, "cmCtrl", cm_ctrl_bytes(k.nBlocks), (void**)&o->marked, k.s);
}

static int cm_encode(const EcEnc& k, EcStaged* o)
{
    if (int r = binary_staging(k, o)) return r;
    launch_cm_encode(k.s, k.view, k.origLen, k.copyThreshold, k.nBlocks, k.maxChunks, k.desc, o->hdr, cm_stage_stride(k.S), o->marked);
    return 0;
}

// (the predictor's tables, for as many blocks as the budget lets run at once, tpaq.hip)
static int tpaq_encode(const EcEnc& k, EcStaged* o)
{
    if (int r = binary_staging(k, o)) return r;
    const size_t tb = tpaq_table_bytes(k.rbsz, (u32)k.S, k.extra);
    if (int r = ws_get(k.c, "tpaqTables", tb * (size_t)tpaq_slice_blocks(tb, k.nBlocks), &o->tables, k.s)) return r;
    launch_tpaq_encode(k.s, k.extra, k.view, k.origLen, k.copyThreshold, k.nBlocks, k.maxChunks, k.desc, o->hdr, cm_stage_stride(k.S), o->marked, o->tables, k.rbsz, (u32)k.S);
    return 0;
}

static int tpaq_again(const EcEnc& k, const EcStaged& o, CmBigAlloc bigAlloc, void* user)
{
    return launch_tpaq_encode_again(k.s, k.extra, k.view, k.origLen, k.copyThreshold, k.nBlocks, k.maxChunks, k.desc, o.hdr, cm_stage_stride(k.S), o.marked, bigAlloc, user,
                                    o.tables, k.rbsz, (u32)k.S);
}

// (tables per lane; a valid block is at most S bytes)
static int tpaq_decode(const EcDec& k)
{
    const size_t tb = tpaq_table_bytes(k.rbsz, (u32)k.S, k.extra);
    void* d_tables;
    if (int r = ws_get(k.c, lane_ws("tpaqTables", k.lane), tb * (size_t)tpaq_slice_blocks(tb, k.nb), &d_tables, k.s)) return r;
    launch_tpaq_decode(k.s, k.extra, k.src, k.blk, k.nb, k.dst, d_tables, k.rbsz, (u32)k.S);
    return 0;
}

static const EcInfo EC[] = {
    // (nothing is staged: the 64 bytes keep the one buffer under its name)
    { .id = KNZ_E_NONE, .entChunk = ENT_CHUNK,
      .encode = [](const EcEnc& k, EcStaged* o) {
          if (int r = ws_get(k.c, "chunkTmp", 64, (void**)&o->hdr, k.s)) return r;
          launch_none_encode(k.s, k.view, k.nBlocks, k.maxChunks, k.desc); return 0; },
      .decode = [](const EcDec& k) { launch_none_decode(k.s, k.src, k.blk, k.nb, k.dst); return 0; } },
    { .id = KNZ_E_ANS0, .entChunk = ENT_CHUNK,
      .encode = [](const EcEnc& k, EcStaged* o) {
          uint2* d_encTab;
          if (int r = ws_get(k.c, "chunkTmp", (size_t)TMP_STRIDE * k.nSlots, (void**)&o->hdr, k.s)) return r;
          if (int r = ws_get(k.c, "encTab", sizeof(uint2) * 256 * k.nSlots, (void**)&d_encTab, k.s)) return r;
          launch_ans0_encode(k.s, k.view, k.nBlocks, k.maxChunks, k.desc, d_encTab, o->hdr); return 0; },
      .decode = [](const EcDec& k) {
          void* d_meta;
          if (int r = ws_get(k.c, lane_ws("ansDecChunks", k.lane), ans0_dec_chunk_bytes() * k.nSlots, &d_meta, k.s)) return r;
          launch_ans0_decode(k.s, k.src, k.blk, k.nb, k.maxChunks, d_meta, k.dst); return 0; } },
    // order-1 rANS writes 256 frequency tables per 4 MiB chunk (<= 3498 bits each), however small the block
    { .id = KNZ_E_ANS1, .entChunk = ANS1_CHUNK, .slots = ANS1_SLOTS,
      .bound = [](size_t n, size_t nb) { return default_bound(n, nb) + (n / ANS1_CHUNK + nb) * 256 * (size_t)HDR_BYTES; },
      .encode = ans1_encode, .decode = ans1_decode },
    { .id = KNZ_E_HUFFMAN, .entChunk = ENT_CHUNK,
      .encode = [](const EcEnc& k, EcStaged* o) {
          if (int r = ws_get(k.c, "chunkTmp", (size_t)TMP_STRIDE * k.nSlots, (void**)&o->hdr, k.s)) return r;
          launch_huffman_encode(k.s, k.view, k.nBlocks, k.maxChunks, k.desc, o->hdr); return 0; },
      .decode = [](const EcDec& k) {
          void* d_meta;
          if (int r = ws_get(k.c, lane_ws("hufDecChunks", k.lane), huffman_dec_chunk_bytes() * k.nSlots, &d_meta, k.s)) return r;
          launch_huffman_decode(k.s, k.src, k.blk, k.nb, k.maxChunks, d_meta, k.dst, k.bsVersion); return 0; } },
    { .id = KNZ_E_FPAQ, .entChunk = 4u << 20,
      .encode = fpaq_encode,
      .decode = [](const EcDec& k) { launch_fpaq_decode(k.s, k.src, k.blk, k.nb, k.dst); return 0; } },
    // RANGE: a chunk of c bytes leaves at most c + c / 64 + 2 units of 28 bits and 60 bits of low (range.hip), behind its header
    { .id = KNZ_E_RANGE, .entChunk = RANGE_CHUNK,
      .bound = [](size_t n, size_t nb) { return 4 * (n + n / 64) + nb * 64 + (n / RANGE_CHUNK + nb) * (HDR_BYTES + 64) + 4096; },
      .encode = [](const EcEnc& k, EcStaged* o) {
          u32* d_cumFreq;
          if (int r = ws_get(k.c, "chunkTmp", (size_t)RANGE_STRIDE * k.nSlots, (void**)&o->hdr, k.s)) return r;
          if (int r = ws_get(k.c, "rangeCumFreq", sizeof(u32) * 256 * k.nSlots, (void**)&d_cumFreq, k.s)) return r;
          o->hdrStride = RANGE_STRIDE;
          launch_range_encode(k.s, k.view, k.origLen, k.copyThreshold, k.nBlocks, k.maxChunks, k.desc, d_cumFreq, o->hdr); return 0; },
      .decode = [](const EcDec& k) { launch_range_decode(k.s, k.src, k.blk, k.nb, k.dst, k.framing); return 0; } },
    // (the binary coders: the chunk length depends on the block's own length, so a block is ONE chunk of the framing's arithmetic that
    // owns cm_max_chunks(S) slots; the slots a block does not use stay zero and add nothing)
    { .id = KNZ_E_CM, .entChunk = 0x80000000u, .slotsOf = cm_max_chunks, .twoTier = true, .bound = binary_bound,
      .encode = cm_encode,
      .again = [](const EcEnc& k, const EcStaged& o, CmBigAlloc bigAlloc, void* user) {
          return launch_cm_encode_again(k.s, k.view, k.origLen, k.copyThreshold, k.nBlocks, k.maxChunks, k.desc, o.hdr, cm_stage_stride(k.S), o.marked, bigAlloc, user); },
      .decode = [](const EcDec& k) { launch_cm_decode(k.s, k.src, k.blk, k.nb, k.dst); return 0; } },
    { .id = KNZ_E_TPAQ, .entChunk = 0x80000000u, .slotsOf = cm_max_chunks, .twoTier = true, .extra = 0, .bound = binary_bound,
      .encode = tpaq_encode, .again = tpaq_again, .decode = tpaq_decode },
    { .id = KNZ_E_TPAQX, .entChunk = 0x80000000u, .slotsOf = cm_max_chunks, .twoTier = true, .extra = 1, .bound = binary_bound,
      .encode = tpaq_encode, .again = tpaq_again, .decode = tpaq_decode },
};

static const EcInfo* ec_info(int id) { for (const EcInfo& e : EC) if (e.id == id) return &e; return nullptr; }

size_t knz_hip_encode_bound(const knz_params* p, size_t n)
{
    const size_t bs = (size_t)p->block_size;
    const size_t nb = (n + bs - 1) / bs + 1;
    const EcInfo* ec = ec_info(p->entropy_type);
    return ec && ec->bound ? ec->bound(n, nb) : default_bound(n, nb);
}

// A chain as a batch entry point takes it: the ids in stream order, and the table row of every stage the device runs (nullptr: NONE, or
// one of the leading stages the host runs), and the entropy coder's row
struct Chain { int n = 0; int tok[8]; const XfInfo* xf[8]; const EcInfo* ec = nullptr; };

// The checks every batch entry point makes: the chain's ids (host stages first, device stages behind them), LZ / LZX behind PACK (encoding
// only), the entropy id, the checksum width
static int parse_chain(Ctx* c, const knz_params* p, int nHosted, bool encoding, Chain* ch)
{
    ch->n = count_transforms(p->transform_type, ch->tok);
    if (nHosted < 0 || nHosted > ch->n) return fail(c, KNZ_ERR_INVALID_PARAM, "host stage count %d does not fit the chain", nHosted);
    for (int i = 0; i < ch->n; i++) {
        const int t = ch->tok[i];
        ch->xf[i] = nullptr;
        if (i < nHosted) { if (!host_stage_id(t)) return fail(c, KNZ_ERR_INVALID_CODEC, "transform id %d is no host stage", t); }
        else if (t != KNZ_T_NONE && (ch->xf[i] = xf_info(t)) == nullptr) return unsupported(c, t);
    }
    for (int i = 0, typed = 0; encoding && i < ch->n; i++) {
        if (ch->xf[i] == nullptr) continue;
        if (typed && ch->xf[i]->ignoresType) return fail(c, KNZ_ERR_INVALID_CODEC, "LZ / LZX behind PACK is not implemented on device");
        typed |= ch->xf[i]->setsType;
    }
    if ((ch->ec = ec_info(p->entropy_type)) == nullptr) return fail(c, KNZ_ERR_INVALID_CODEC, "entropy id %d not implemented on device", p->entropy_type);
    if (p->checksum_bits != 0 && p->checksum_bits != 32 && p->checksum_bits != 64) return fail(c, KNZ_ERR_INVALID_PARAM, "checksum must be 0, 32 or 64");
    return 0;
}

// buffer size of a block of n bytes: the largest any prefix of the chain may write (TransformSequence::getMaxEncodedLength)
static int seq_required(const Chain& ch, int n)
{
    int req = n;
    for (int i = 0; i < ch.n; i++) req = std::max(req, knz_max_encoded_len(ch.tok[i], req));
    return req;
}

// stride of a chain's two workspaces for blocks of n bytes. The chain's bound is what the reference gives the task's "buffer", and a
// stage in even position may fill it: ZRLT in front writes up to requiredSize for a block without zeros, more than its own
// getMaxEncodedLength. The stage behind it writes into the task's "data" (256 KiB or more, model_capacities) and asks for its own bound over
// that longer input (LZP: n + n / 64, ROLZX and SRT: n + 1024, MM: n + n / 16), so with two stages or more the stride is the chain's
// bound of the chain's bound. A capacity is cut to the stride (k_seq_fwd_prepare); cut to the bound alone, ZRLT+LZP, ZRLT+ROLZX,
// ZRLT+SRT and ZRLT+MM refused blocks in second position that the reference transforms (tests/test_gpu_pairs.py).
static int seq_stride(const Chain& ch, int n)
{
    int stages = 0;
    for (int i = 0; i < ch.n; i++) stages += ch.tok[i] != KNZ_T_NONE;
    const int req = seq_required(ch, n);
    return stages < 2 ? req : seq_required(ch, req);
}

static size_t chain_scratch_u32(const Chain& ch, bool forward, int nBlocks, u32 maxLen)
{
    size_t most = 0;
    for (int i = 0; i < ch.n; i++) if (ch.xf[i]) most = std::max(most, scratch_u32(forward ? ch.xf[i]->fwd : ch.xf[i]->inv, nBlocks, maxLen));
    return most;
}

// part k of n parts of nBlocks blocks: runs of consecutive blocks, the first nBlocks % n one block longer
static void cut(int nBlocks, int n, int k, int* first, int* count)
{
    *first = k * (nBlocks / n) + std::min(k, nBlocks % n);
    *count = nBlocks / n + (k < nBlocks % n ? 1 : 0);
}

using PartFn = std::function<int(int, hipStream_t)>;

// Parts 0..n-1 of one piece of work side by side: part 0 on `s`, part k on side stream k-1, which starts behind what is queued on `s`.
// prepare(k, q) (optional: workspaces) runs for every part on the caller's thread, then run(k, q): there as well, or with `threads` on helper
// thread k-1 for k >= 1. Every side stream is joined into `s` before the return, whatever failed; after a failure the streams are also
// synchronised, so that no kernel is left running on a lane's workspaces when the caller releases the context. Returns the first failure.
static int fork_join(Ctx* c, hipStream_t s, int n, bool threads, const PartFn& run, const PartFn& prepare = nullptr)
{
    if (n == 1) { const int r = prepare ? prepare(0, s) : 0; return r ? r : run(0, s); }
    HIPCHK(c, hipSetDevice(c->device));                          // the side streams belong to the context's device
    for (int k = 1; k < n; k++)
        if (c->stream2[k - 1] == nullptr) HIPCHK(c, hipStreamCreateWithFlags(&c->stream2[k - 1], hipStreamNonBlocking));
    for (hipEvent_t* e : { &c->evFork, &c->evJoin[0], &c->evJoin[1], &c->evJoin[2] })
        if (*e == nullptr) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    const hipStream_t q[4] = { s, c->stream2[0], c->stream2[1], c->stream2[2] };
    HIPCHK(c, hipEventRecord(c->evFork, s));
    int rc = 0;
    auto check = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == 0) rc = fail(c, -1, "%s failed: %s", what, hipGetErrorString(e)); };
    for (int k = 1; k < n && rc == 0; k++) check(hipStreamWaitEvent(q[k], c->evFork, 0), "waiting for the fork");
    for (int k = 0; k < n && rc == 0 && prepare; k++) rc = prepare(k, q[k]);
    if (rc == 0 && !threads) {
        for (int k = 0; k < n && rc == 0; k++) rc = run(k, q[k]);
    } else if (rc == 0) {
        int part[4] = { 0, 0, 0, 0 }, begun = 1;
        try {
            for (; begun < n; begun++)
                c->helpers[begun - 1].run([&, k = begun] {
                    part[k] = hipSetDevice(c->device) == hipSuccess ? run(k, q[k]) : fail(c, -1, "a helper thread cannot select the device");
                });
        } catch (...) {
            rc = fail(c, -1, "cannot start a helper thread");
        }
        if (rc == 0) part[0] = run(0, s);
        for (int k = 1; k < begun; k++) c->helpers[k - 1].wait();
        for (int k = 0; k < n && rc == 0; k++) rc = part[k];
    }
    for (int k = 1; k < n; k++) {                                // `s` continues behind every side stream
        hipError_t e = hipEventRecord(c->evJoin[k - 1], q[k]);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, c->evJoin[k - 1], 0);
        check(e, "joining a side stream");
    }
    if (rc) for (int k = 0; k < n; k++) hipStreamSynchronize(q[k]);
    return rc;
}

// The BWT stages of a batch in several parts at once. A suffix sort (and the inverse's list ranking) is a long sequence of launches
// with host read-backs in between and rounds that occupy a fraction of the CUs; the blocks are independent, so the batch is cut
// into KNZ_BWT_SPLIT (default 3, 1 = off, at most 4; 26 blocks of 8 MiB: 63.7 / 60.4 / 59.9 / 60.3 ms per step with 1 / 2 / 3 / 4) runs of blocks: the caller's thread drives the first on the context's stream,
// helper threads drive the others on streams of their own, each with its own scratch and read-back area. Not while per-kernel
// timing is on (the timing hooks belong to the caller's thread).
static int bwt_parts_wanted(const Ctx* c, int nBlocks)
{
    if (c->profiling) return 1;
    int parts = bwt_split_knob().load();
    const int least = bwt_part_min_knob().load();
    while (parts > 1 && nBlocks < least * parts) parts--;        // at least `least` blocks per part
    return parts;
}

// One stage over the batch `st` on stream s. lane -1: a whole batch, which a stage that allows it runs as parts side by side (part k with
// lane k's scratch and read-back area); lane k >= 0: decode lane k, not split further.
static int run_stage(Ctx* c, hipStream_t s, const XfInfo& x, bool forward, const XfStage& st, int lane = -1)
{
    const XfDir& d = forward ? x.fwd : x.inv;
    const int parts = (lane < 0 && d.split != NO_SPLIT) ? bwt_parts_wanted(c, st.nBlocks) : 1;
    XfStage part[4];
    void* ws[4] = { nullptr, nullptr, nullptr, nullptr };
    size_t bytes[4] = { 0, 0, 0, 0 };
    for (int k = 0; k < parts; k++) {
        int first, nb;
        cut(st.nBlocks, parts, k, &first, &nb);
        part[k] = st;
        part[k].nBlocks = nb;
        part[k].src += first; part[k].dst += first; part[k].len += first; part[k].cap += first; part[k].ok += first; part[k].newLen += first;
    }
    auto at = [&](int k) { return lane < 0 ? k : lane; };      // the lane whose scratch and read-back area part k uses
    return fork_join(c, s, parts, d.split == SPLIT_THREADS,
                     [&](int k, hipStream_t q) { return d.launch({ c, q, part[k], ws[k], bytes[k], lane_pinned(c, at(k)) }); },
                     [&](int k, hipStream_t q) {
                         if (d.wsBytes == nullptr && d.wsBytesOf == nullptr) return 0;
                         bytes[k] = d.wsBytesOf ? d.wsBytesOf(part[k]) : d.wsBytes(part[k].nBlocks, st.maxLen);
                         return ws_get(c, lane_ws(x.ws, at(k)), bytes[k], &ws[k], q);
                     });
}

// ------------------------------------------------------------------------------------------------
// encode
// ------------------------------------------------------------------------------------------------
// The workspaces of a batch of many streams are blocks x the stride of the longest block (two of them, seq_alloc). A caller that keeps
// blocks x longest block below 2 GiB (the documented limit, include/knz_hip.h) stays below this whatever the chain adds to the stride.
constexpr u64 STREAMS_MAX_WORK = (u64)1 << 32;

// A batch of many streams as the encoder takes it (knz_hip_encode_streams builds it): the blocks of all streams in stream order, block b
// at d_in + inOff[b] with len[b] bytes, stream i owning the blocks [first[i], first[i + 1]). The d_* arrays are one upload.
struct EncTab {
    int nItems = 0, nBlocks = 0;
    u32 maxLen = 0;                            // the longest block
    std::vector<u32> first, len;               // host copies (the capacity model runs there)
    const u64* d_inOff = nullptr; const u32* d_len = nullptr; const u32* d_itemOf = nullptr; const StreamEnc* d_st = nullptr; const u8* d_pro = nullptr;
    StreamOut* d_res = nullptr; u64* d_excl = nullptr;
    std::vector<StreamOut> res;                // OUT: where the streams lie
};

// What an entry point asks of the encoder. The defaults are a framed batch of one stream that starts with block 0, without a prologue.
struct EncJob {
    const knz_params* p = nullptr;
    const uint8_t* d_in = nullptr; size_t n = 0;           // (many streams: all their bytes)
    const uint8_t* prologue = nullptr; uint32_t prologueBits = 0;      // host bytes in front of the first block (many streams: unused, every stream has its own)
    int framing = 1;                                       // 0: the bare entropy stage over one buffer (knz_hip_entropy_encode_bs)
    int finish = 0;                                        // the end marker behind the blocks
    int64_t firstBlock = 0;                                // the first block's id in its stream (many streams count from 0)
    uint8_t* d_out = nullptr; size_t outCap = 0;
    uint64_t* outBits = nullptr;                           // OUT: the bits written (many streams: 8 * the bytes of d_out in use); nullptr: no wait for the assembly
    const knz_host_stages* hs = nullptr;                   // one block whose leading stages the host has run
    u32 streamBlockSize = 0;                               // block size of the stream the buffer belongs to, where p->block_size is not it (per-stage calls)
    EncTab* tab = nullptr;                                 // the batch holds many streams
};

// Destination capacities the reference would present (io/CompressedOutputStream.cpp:141,461-462,733-739): block i of a stream runs on
// buffer slot i % jobs; "data" of slot 0 is max(bs + bs/8, 256 KiB), of the others max(bs + bs/64, 64 KiB); "buffer" grows to the largest
// requiredSize seen on the slot. Host arithmetic only: bufCap[b] and dataCap[b] of the nBlocks blocks of one stream whose first has the id
// firstBlock -- len[b] bytes each, or with len == nullptr n bytes cut into blocks of bs --, or with `first` (every stream's first block, and
// one entry more) of many streams, each of which starts with fresh buffers and counts its blocks from 0.
static void model_capacities(const Chain& ch, int jobs, u32 bs, int64_t firstBlock, int nBlocks, size_t n, const u32* len, const u32* first,
                             u32* bufCap, u32* dataCap)
{
    jobs = (jobs <= 0) ? 1 : (jobs > 64 ? 64 : jobs);
    u32 slotBuf[64] = { 0 };
    const u32 full = (u32)seq_required(ch, (int)bs);
    for (int64_t b = 0, it = 0; b < nBlocks; b++) {
        if (first) {
            const int64_t was = it;
            while ((int64_t)first[it + 1] <= b) it++;
            if (it != was) std::fill(slotBuf, slotBuf + jobs, 0u);
        }
        const int64_t gid = first ? b - (int64_t)first[it] : firstBlock + b;
        const int slot = (int)(gid % jobs);
        const u32 l = len ? len[b] : (u32)(((size_t)(b + 1) * bs <= n) ? bs : n - (size_t)b * bs);      // (the reference sizes its buffers by the block as read)
        const u32 req = (u32)seq_required(ch, (int)l);
        // a slot's buffer is at least what a full block needed earlier on that slot, and what this block needs
        u32 bufc = slotBuf[slot];
        if (gid >= jobs && bufc < full) bufc = full;
        if (bufc < req) bufc = req;
        slotBuf[slot] = bufc;
        const u32 datac = (slot == 0) ? std::max(bs + (bs >> 3), 256u * 1024u) : std::max(bs + (bs >> 6), 65536u);
        bufCap[b] = bufc;
        dataCap[b] = std::max(datac, req);
    }
}

// One batch through the transforms, the entropy coder and the bit assembly, phase by phase (run). Four kinds of request share it: a
// framed batch, one hosted block (hs), many streams (tab), and the bare entropy stage of the per-stage calls (framing 0).
struct Encoder {
    Ctx* c; const EncJob& j;
    ProfInstall prof;
    const knz_params* p; const knz_host_stages* hs; EncTab* tab; hipStream_t s; u32 bs; PinnedWords pin;
    Chain ch; int nHosted = 0, nBlocks = 0;
    bool realStages = false, wantType = false, direct = false;      // a stage other than NONE; a device stage reads the per-block data type; NullTransforms only
    FrameParams fp; u64* d_total = nullptr;
    u64 S = 0; SeqWs w;
    u32* d_origLen = nullptr; BlockInfo* d_info = nullptr; u64* d_sums = nullptr;
    EcEnc enc; EcStaged staged; u32 slotMul = 1;

    Encoder(Ctx* ctx, const EncJob& job) : c(ctx), j(job), prof(ctx), p(job.p), hs(job.hs), tab(job.tab), s(ctx->stream), bs((u32)job.p->block_size), pin(ctx) {}

    const u64* in_off() const { return tab ? tab->d_inOff : nullptr; }
    const u32* len_tab() const { return tab ? tab->d_len : nullptr; }
    size_t min_out() const { return ((size_t)j.prologueBits + 7) / 8 + 16; }

    // The request is one the phases can take: the chain, nBlocks and the frame parameters are set. Nothing is launched.
    int check()
    {
        HIPCHK(c, hipSetDevice(c->device));
        if ((reinterpret_cast<uintptr_t>(j.d_in) & 15) || (reinterpret_cast<uintptr_t>(j.d_out) & 15))
            return fail(c, KNZ_ERR_INVALID_PARAM, "device buffers must be 16-byte aligned");
        if (j.framing && (bs < 1024 || bs > (1u << 30) || (bs & 15))) return fail(c, KNZ_ERR_INVALID_PARAM, "invalid block size %u", bs);
        nHosted = hs ? hs->stages : 0;
        if (int r = parse_chain(c, p, nHosted, true, &ch)) return r;
        for (int i = 0; i < ch.n; i++) { realStages |= ch.tok[i] != KNZ_T_NONE; wantType |= ch.xf[i] && ch.xf[i]->setsType; }
        // (what the phases behind rely on. No public entry point builds such a request: the per-stage entropy calls have no transform, the
        // per-stage transform calls go through transform_host and never come here)
        if (!j.framing && realStages) return fail(c, KNZ_ERR_INVALID_PARAM, "a call without framing takes no transform");
        nBlocks = tab ? tab->nBlocks : (j.n == 0) ? 0 : (int)((j.n + bs - 1) / bs);
        if (hs) {
            // one block, in the length the host stages left it (never longer than the block it came from)
            if (nBlocks != 1 || hs->orig_len > bs || j.n > hs->orig_len + 8192u) return fail(c, KNZ_ERR_INVALID_PARAM, "a hosted call takes exactly one block");
            if ((hs->orig_len <= 15) != (j.n <= 15) || (hs->orig_len <= 15 && hs->applied_mask)) return fail(c, KNZ_ERR_INVALID_PARAM, "copy blocks go through no stage");
        }
        // device-side positions of a batch are 32-bit (suffix array slots, bit offsets inside staging areas): a batch
        // is limited to 2 GiB of input; the host layers split larger inputs into several calls
        if (j.n > (size_t)0x7FFFFFFF - 8ull * (size_t)(nBlocks + 1) * 1056) return fail(c, KNZ_ERR_INVALID_PARAM, "batch of %zu bytes exceeds the 2 GiB per-call limit", j.n);
        if ((j.prologueBits + 7) / 8 > 200) return fail(c, KNZ_ERR_INVALID_PARAM, "prologue too long");
        if (j.outCap < min_out()) return fail(c, KNZ_ERR_WRITE_FILE, "output buffer too small");
        fp.framing = j.framing; fp.nTransforms = ch.n; fp.checksumBits = p->checksum_bits; fp.finish = j.finish; fp.prologueBits = j.prologueBits;
        return ws_get(c, "total", 64, (void**)&d_total, s);
    }

    // No block: the output is the prologue (every stream's own) and, where asked for, the end marker. Synchronises the stream.
    int empty()
    {
        if (tab) {
            launch_stream_frame(s, nullptr, nullptr, nullptr, nullptr, 0, tab->d_st, tab->nItems, fp, tab->d_excl, tab->d_res, d_total);
            if (int r = read_total(false)) return r;
            return place();
        }
        HIPCHK(c, hipMemsetAsync(j.d_out, 0, min_out(), s));
        if (int r = prologues()) return r;
        HIPCHK(c, hipStreamSynchronize(s));
        if (j.outBits) *j.outBits = (u64)j.prologueBits + ((j.framing && j.finish) ? 8 : 0);
        return 0;
    }

    // The per-block arrays and the chain's workspaces of stride S. Queued: the blocks' lengths (the direct path sets them with its one
    // launch, transforms) and the checksums of the ORIGINAL bytes (io/CompressedOutputStream.cpp:675-682).
    int bookkeeping()
    {
        if (int r = ws_get(c, "origLen", sizeof(u32) * nBlocks, (void**)&d_origLen, s)) return r;
        if (int r = ws_get(c, "info", sizeof(BlockInfo) * nBlocks, (void**)&d_info, s)) return r;
        const int maxIn = tab ? (int)tab->maxLen : (int)((j.n < bs) ? j.n : bs);
        S = ((u64)seq_stride(ch, maxIn) + 255) & ~255ull;
        if (tab && (u64)nBlocks * S > STREAMS_MAX_WORK) return fail(c, KNZ_ERR_INVALID_PARAM, "%d blocks with a longest block of %d bytes exceed the workspace limit of a call (blocks x longest block <= 2 GiB): split the call", nBlocks, maxIn);
        if (int r = seq_alloc(c, nBlocks, S, realStages, chain_scratch_u32(ch, true, nBlocks, (u32)S), &w, -1, s)) return r;
        w.a.origLen = d_origLen;
        direct = !realStages && !p->checksum_bits;
        if (!direct) launch_init_blocks(s, j.n, bs, nBlocks, d_origLen, w.a.len, len_tab());
        if (!p->checksum_bits) return 0;
        if (int r = ws_get(c, "sums", sizeof(u64) * nBlocks, (void**)&d_sums, s)) return r;
        if (hs) {
            // (the host computed the checksum before its stages ran)
            *pin.hostedSum() = hs->checksum;
            HIPCHK(c, hipMemcpyAsync(d_sums, pin.hostedSum(), sizeof(u64), hipMemcpyHostToDevice, s));
        } else {
            launch_block_ptrs(s, j.d_in, bs, nBlocks, w.d_viewPtr, in_off());
            launch_xxhash(s, w.d_viewPtr, d_origLen, nBlocks, p->checksum_bits, d_sums);
        }
        return 0;
    }

    // The capacities of the reference's buffers (model_capacities) on the device, for chains with a stage. Synchronises the stream: the
    // arrays leave through the pinned area, whose words the stages and the framing use from here on (PinnedWords).
    int capacities()
    {
        if (!realStages) return 0;
        if ((size_t)nBlocks * 8 > c->pinnedCap) return fail(c, KNZ_ERR_INVALID_PARAM, "too many blocks in one batch (%d)", nBlocks);
        u32* hEven = pin.caps(); u32* hOdd = hEven + nBlocks;
        model_capacities(ch, p->jobs, bs, j.firstBlock, nBlocks, j.n, tab ? tab->len.data() : hs ? &hs->orig_len : nullptr, tab ? tab->first.data() : nullptr,
                         hEven, hOdd);
        HIPCHK(c, hipMemcpyAsync(w.d_capEven, hEven, sizeof(u32) * nBlocks, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(w.d_capOdd, hOdd, sizeof(u32) * nBlocks, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return 0;
    }

    // The per-block data type, where a device stage reads it: preset from the block's magic, or what the host stages left
    int data_types()
    {
        if (!wantType) return 0;
        if (hs) HIPCHK(c, hipMemsetAsync(w.a.dtype, hs->reserved <= 9 ? (int)hs->reserved : 0, (size_t)nBlocks, s));
        else launch_seq_fwd_dtype(s, w.a, nBlocks, j.d_in, bs, in_off());
        return 0;
    }

    // The chain over the batch: w.d_viewPtr and w.a.len are what the entropy coder reads, w.a.skip the stages that refused a block. The BWT
    // and BWTS stages synchronise the stream between their rounds (XF).
    int transforms()
    {
        if (direct) { launch_seq_fwd_direct(s, w.a, d_origLen, j.n, bs, nBlocks, ch.n, j.d_in, w.d_viewPtr, in_off(), len_tab()); return 0; }
        for (int i = 0; i < ch.n; i++) {
            launch_seq_fwd_prepare(s, w.a, nBlocks, i, j.d_in, bs, w.A, w.B, S, in_off());
            if (i < nHosted) {
                launch_seq_fwd_hosted(s, w.a, nBlocks, i, (hs->applied_mask >> i) & 1u);
                continue;
            }
            if (ch.xf[i] == nullptr) {
                launch_seq_fwd_null(s, w.a, nBlocks, i);
                continue;
            }
            XfStage st = xf_stage(w, nBlocks, (u32)S, p->entropy_type);
            st.dtype = wantType ? w.a.dtype : nullptr;
            st.blockSize = j.streamBlockSize ? j.streamBlockSize : bs;
            // (TransformFactory.hpp:290-295: the DNA transform leaves packOnlyDNA in the Context that the chain's later stages are built
            // from, so a PACK anywhere behind it in the same chain refuses what is not DNA as well)
            for (int k = 0; k < i; k++) if (ch.tok[k] == KNZ_T_DNA) st.onlyDNA = 1;
            if (int r = run_stage(c, s, *ch.xf[i], true, st)) return r;
            launch_seq_fwd_commit(s, w.a, nBlocks, i);
        }
        launch_seq_fwd_finish(s, w.a, nBlocks, j.d_in, bs, w.A, w.B, S, w.d_viewPtr, in_off());
        return 0;
    }

    // The coder's launches over the batch (enc); `staged` is what it leaves for the framing, and for a second tier
    int entropy()
    {
        const EcInfo* ec = ch.ec;
        slotMul = ec->slotsOf ? (u32)ec->slotsOf(S) : ec->slots;
        const int chunksPerBlock = (int)((S + ec->entChunk - 1) / ec->entChunk);
        const int maxChunks = chunksPerBlock * (int)slotMul;
        const size_t nSlots = (size_t)nBlocks * maxChunks;
        ChunkDesc* d_desc;
        if (int r = ws_get(c, "desc", sizeof(ChunkDesc) * nSlots, (void**)&d_desc, s)) return r;
        BlockView view;
        view.ptr = w.d_viewPtr; view.len = w.a.len;
        enc = { c, s, view, d_origLen, j.framing ? 15u : 0u, nBlocks, S, chunksPerBlock, maxChunks, nSlots, d_desc,
                j.streamBlockSize ? j.streamBlockSize : bs, ec->extra };
        return ec->encode(enc, &staged);
    }

    // d_total, and with `marked` the count of the blocks that did not fit their staging, in the pinned words. Synchronises the stream.
    int read_total(bool marked)
    {
        if (marked) *pin.marked() = 0;
        HIPCHK(c, hipMemcpyAsync(pin.total(), d_total, sizeof(u64), hipMemcpyDeviceToHost, s));
        if (marked && staged.marked) HIPCHK(c, hipMemcpyAsync(pin.marked(), staged.marked, sizeof(u32), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return 0;
    }

    // The blocks' lengths summed and their places scanned (many streams: the places restart at every stream, and d_total holds the BYTES
    // of output in use), the total read back. Synchronises the stream.
    int sum_and_scan(bool marked)
    {
        launch_block_sum(s, enc.desc, d_info, w.a.len, nBlocks, enc.maxChunks, ch.ec->entChunk, slotMul);
        if (tab) launch_stream_frame(s, d_info, w.a.len, d_origLen, tab->d_itemOf, nBlocks, tab->d_st, tab->nItems, fp, tab->d_excl, tab->d_res, d_total);
        else launch_block_scan(s, d_info, w.a.len, d_origLen, nBlocks, fp, d_total);
        return read_total(marked);
    }

    // Every block's place in the output and the output's size on the host: it must be zero before the OR-assembly and its size is only
    // known on the device, so the total is read back first (8 bytes) and only the used part is cleared (place). Synchronises the stream
    // once, or twice where blocks of a two-tier coder are coded again.
    int frame()
    {
        if (int r = sum_and_scan(true)) return r;
        if (*pin.marked() == 0) return 0;
        // the rare path: blocks that did not fit their staging are coded again into 32 n + 16 bytes each (workspace taken only now),
        // then the lengths are summed again
        struct Big { Ctx* c; hipStream_t s; int rc; } big = { c, s, 0 };
        auto bigAlloc = [](void* user, size_t bytes) -> void* {
            Big* g = static_cast<Big*>(user);
            void* m = nullptr;
            g->rc = ws_get(g->c, "cmBig", bytes, &m, g->s);
            return g->rc ? nullptr : m;
        };
        const int r = ch.ec->again(enc, staged, bigAlloc, &big);
        if (r == -2) return big.rc;                               // (ws_get has said why)
        if (r < 0) return fail(c, -1, "binary coder: encode failed: %s", hipGetErrorString(hipGetLastError()));
        return sum_and_scan(false);
    }

    // The prologue, or every stream's own, into the cleared output
    int prologues()
    {
        if (tab) { launch_stream_prologues(s, reinterpret_cast<u32*>(j.d_out), tab->d_st, tab->d_res, tab->nItems, tab->d_pro); return 0; }
        if (!j.prologueBits) return 0;
        u8* d_pro;
        if (int r = ws_get(c, "prologue", 256, (void**)&d_pro, s)) return r;
        HIPCHK(c, hipMemcpyAsync(d_pro, j.prologue, (j.prologueBits + 7) / 8, hipMemcpyHostToDevice, s));
        launch_put_prologue(s, reinterpret_cast<u32*>(j.d_out), d_pro, j.prologueBits);
        return 0;
    }

    // The output behind the framing: room check, the one clearing of what is used (many streams: the padding between them included),
    // prologues, assembly, and what the caller gets back. Many streams: synchronises the stream (where the streams lie is read back);
    // one stream: only where the caller asks for the bit count.
    int place()
    {
        const u64 total = *pin.total();                           // bits of the one stream, or bytes of all streams
        const size_t used = tab ? (size_t)total : ((size_t)((total + 7) >> 3) + 8 + 3) & ~(size_t)3;
        if (used > j.outCap) return fail(c, KNZ_ERR_WRITE_FILE, "output buffer too small: need %zu have %zu", used, j.outCap);
        {
            ProfScope ps(c, "memset_out");
            if (used) HIPCHK(c, hipMemsetAsync(j.d_out, 0, used, s));
        }
        if (int r = prologues()) return r;
        if (nBlocks) launch_assemble(s, enc.desc, d_info, w.a.len, d_origLen, w.a.skip, d_sums, staged.hdr, nBlocks, enc.maxChunks, ch.ec->entChunk, slotMul, staged.hdrStride, fp,
                                     reinterpret_cast<u32*>(j.d_out));
        if (!tab) {
            HIPCHK(c, hipGetLastError());
            if (j.outBits) {
                HIPCHK(c, hipStreamSynchronize(s));
                *j.outBits = total;
            }
            return 0;
        }
        if (j.outBits) *j.outBits = 8 * total;
        tab->res.resize((size_t)tab->nItems);
        if (tab->nItems) HIPCHK(c, hipMemcpyAsync(tab->res.data(), tab->d_res, sizeof(StreamOut) * (size_t)tab->nItems, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipGetLastError());
        return 0;
    }

    int run()
    {
        if (int r = check()) return r;
        if (nBlocks == 0) return empty();
        if (int r = bookkeeping()) return r;
        if (int r = capacities()) return r;
        if (int r = data_types()) return r;
        if (int r = transforms()) return r;
        if (int r = entropy()) return r;
        if (int r = frame()) return r;
        return place();
    }
};

int knz_hip_encode_blocks(knz_ctx* ctx, const knz_params* p, const uint8_t* d_in, size_t n, const uint8_t* prologue,
                          uint32_t prologue_bits, int64_t first_block_id, int finish, uint8_t* d_out, size_t out_cap,
                          uint64_t* out_bits)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    EncJob j;
    j.p = p; j.d_in = d_in; j.n = n; j.prologue = prologue; j.prologueBits = prologue_bits; j.firstBlock = first_block_id; j.finish = finish;
    j.d_out = d_out; j.outCap = out_cap; j.outBits = out_bits;
    return Encoder(c, j).run();
}

int knz_hip_encode_block_hosted(knz_ctx* ctx, const knz_params* p, const knz_host_stages* hs, const uint8_t* d_in, size_t n, const uint8_t* prologue,
                                uint32_t prologue_bits, int64_t first_block_id, int finish, uint8_t* d_out, size_t out_cap, uint64_t* out_bits)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    if (!hs) return fail(c, KNZ_ERR_INVALID_PARAM, "no host stage record");
    EncJob j;
    j.p = p; j.d_in = d_in; j.n = n; j.prologue = prologue; j.prologueBits = prologue_bits; j.firstBlock = first_block_id; j.finish = finish;
    j.d_out = d_out; j.outCap = out_cap; j.outBits = out_bits; j.hs = hs;
    return Encoder(c, j).run();
}

// ------------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------------
// A batch of many streams as the decoder takes it (knz_hip_decode_streams builds it): d_sd is the upload of the items, d_walk room for
// one StreamWalk per stream and one more. The per-stream verdicts go back into `items`.
struct DecTab {
    int nItems = 0;
    u32 maxUnit = 0;                           // the longest block any item has room for: min(block size, out_cap), at most
    knz_item* items = nullptr;
    const StreamDec* d_sd = nullptr; StreamWalk* d_walk = nullptr;
};

// What an entry point asks of the decoder. The defaults are the framed blocks of one stream from bit 0, as many as the output holds.
struct DecJob {
    const knz_params* p = nullptr;
    const uint8_t* d_in = nullptr; uint64_t inBits = 0;    // (many streams: the bits of d_in that any stream reaches)
    uint64_t startBit = 0; int64_t maxBlocks = 0;          // (many streams: unused, every stream has its own start)
    int framing = 1; u32 rawLen = 0;                       // 0: the bare entropy stage of one buffer of rawLen bytes (knz_hip_entropy_decode_bs)
    uint8_t* d_out = nullptr; size_t outCap = 0;
    int nHosted = 0;                                       // leading stages the caller undoes on the host after the call
    u32 streamBlockSize = 0;                               // as EncJob's
    DecTab* tab = nullptr;                                 // the batch holds many streams: each gets its own verdict, and a stream's failure is no failure of the call
};

// What the decoder reports of one stream (of many streams nothing: DecTab::items). An entry point copies out what its ABI has.
struct DecResult {
    bool walked = false;                                   // endBit and blocksDone hold: the walk has passed, whatever failed behind it
    u64 endBit = 0; int64_t blocksDone = 0;
    u64 outBytes = 0;                                      // of a call that succeeds
    int32_t rawDecoded = 0; u64 usedBits = 0;              // the first block's bytes, or -1 where a call without framing cannot decode it; the bits its decoder used
    u32 skipOut = 0xFF; u64 sumOut = 0;                    // the first block's skip flags (0xFF: a copy block, or none) and stored checksum
};

// One batch through the walk, the entropy decoder and the inverse chain, phase by phase (run)
struct Decoder {
    Ctx* c; const DecJob& j; DecResult& res;
    ProfInstall prof;
    const knz_params* p; DecTab* tab; hipStream_t s; u32 bs; PinnedWords pin;
    Chain ch; int bsVersion = 6; BitSrc src;
    u32 realMask = 0; bool lanesOk = true;                   // the device's stages; every one of them may run in lanes
    DecBlock* d_blocks = nullptr; int nBlocks = 0;
    std::vector<StreamWalk> sw;                              // many streams: every stream's first slot, block count and verdict of the walk
    u64 *d_outOff = nullptr, *d_room = nullptr;              // many streams: every block's place in d_out and the room behind it
    u32 unit = 0; u64 S = 0, outStride = 0; int maxChunks = 0, lanes = 1;
    std::vector<DecBlock> hb;                                // the blocks as the device left them

    Decoder(Ctx* ctx, const DecJob& job, DecResult& out) : c(ctx), j(job), res(out), prof(ctx), p(job.p), tab(job.tab), s(ctx->stream), bs((u32)job.p->block_size), pin(ctx) {}

    // The request is one the phases can take: the chain, the bitstream version and the source are set. Nothing is launched.
    int check()
    {
        HIPCHK(c, hipSetDevice(c->device));
        if ((reinterpret_cast<uintptr_t>(j.d_in) & 15) || (reinterpret_cast<uintptr_t>(j.d_out) & 15))
            return fail(c, KNZ_ERR_INVALID_PARAM, "device buffers must be 16-byte aligned");
        if (j.framing && (bs < 1024 || bs > (1u << 30) || (bs & 15))) return fail(c, KNZ_ERR_INVALID_PARAM, "invalid block size %u", bs);
        // (the host stages in front are undone by the caller after the call: for the device they are stages that leave the data alone)
        if (int r = parse_chain(c, p, j.nHosted, false, &ch)) return r;
        for (int i = 0; i < ch.n; i++) if (ch.xf[i]) { realMask |= 1u << (7 - i); lanesOk &= ch.xf[i]->lanes; }
        // (what range() relies on; no public entry point builds such a request, see Encoder::check)
        if (!j.framing && realMask) return fail(c, KNZ_ERR_INVALID_PARAM, "a call without framing takes no transform");
        // bitstream version of the blocks (0 = current). Below 6 the Huffman chunks, the BWT block header and the LZ blocks have their
        // old layouts (HuffmanDecoder.cpp:349-459, BWTBlockCodec.cpp:140-164, LZCodec.cpp:614-760)
        bsVersion = (p->bs_version == 0) ? 6 : p->bs_version;
        if (bsVersion < 0 || bsVersion > 6) return fail(c, KNZ_ERR_STREAM_VERSION, "cannot read bitstream version %d", bsVersion);
        src.words = reinterpret_cast<const u32*>(j.d_in);
        src.nBytes = (j.inBits + 7) >> 3;
        src.nWords = src.nBytes >> 2;
        src.limitBits = j.inBits;
        return 0;
    }

    // nBlocks and every block's place in its stream (d_blocks); many streams: also every block's place and room in the output (d_outOff,
    // d_room) and every item's verdict of the walk; one stream: endBit and blocksDone. Synchronises the stream.
    int walk() { return tab ? walk_streams() : walk_blocks(); }

    // (in two passes, streams.hip: count, scan the counts -- the total sizes the block table --, then fill)
    int walk_streams()
    {
        sw.resize((size_t)tab->nItems + 1);
        launch_walk_streams_count(s, j.d_in, tab->d_sd, tab->nItems, p->checksum_bits, bs, tab->d_walk);
        HIPCHK(c, hipMemcpyAsync(sw.data(), tab->d_walk, sizeof(StreamWalk) * sw.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipGetLastError());
        const u64 all = sw.back().first;
        if (all > (u64)KNZ_STREAMS_MAX_BLOCKS) return fail(c, KNZ_ERR_INVALID_PARAM, "too many blocks in one batch (%llu)", (unsigned long long)all);
        nBlocks = (int)all;
        for (int i = 0; i < tab->nItems; i++) {
            knz_item& it = tab->items[i];
            it.error = sw[(size_t)i].error; it.blocks = (int32_t)sw[(size_t)i].count; it.out_len = 0;
        }
        if (nBlocks == 0) return 0;
        if (int r = ws_get(c, "decBlocks", sizeof(DecBlock) * (size_t)nBlocks, (void**)&d_blocks, s)) return r;
        if (int r = ws_get(c, "decOutOff", sizeof(u64) * (size_t)nBlocks, (void**)&d_outOff, s)) return r;
        if (int r = ws_get(c, "decRoom", sizeof(u64) * (size_t)nBlocks, (void**)&d_room, s)) return r;
        launch_walk_streams_fill(s, j.d_in, tab->d_sd, tab->nItems, p->checksum_bits, bs, tab->d_walk, d_blocks, d_outOff, d_room);
        return 0;
    }

    int walk_blocks()
    {
        int64_t bound = j.framing ? (int64_t)(j.outCap / bs) + 2 : 1;
        if (j.maxBlocks > 0 && j.maxBlocks < bound) bound = j.maxBlocks;
        void* d_walk;
        if (int r = ws_get(c, "decBlocks", sizeof(DecBlock) * (size_t)bound, (void**)&d_blocks, s)) return r;
        if (int r = ws_get(c, "walk", 64, &d_walk, s)) return r;
        launch_walk_blocks(s, src, j.startBit, bound, j.framing, j.rawLen, p->checksum_bits, bs, d_blocks, d_walk);
        HIPCHK(c, hipMemcpyAsync(pin.walk(), d_walk, sizeof(WalkResultHost), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        const WalkResultHost found = *pin.walk();
        if (found.error) return fail(c, found.error, "invalid block framing");
        nBlocks = (int)found.nBlocks;
        res.walked = true; res.endBit = found.endBit; res.blocksDone = nBlocks;
        if (nBlocks && j.framing && (size_t)nBlocks * bs > j.outCap + bs) return fail(c, KNZ_ERR_WRITE_FILE, "output buffer too small");
        return 0;
    }

    // The 2 GiB of a call, by the blocks of one stream or by what the items of many can hold
    int limits()
    {
        if (!tab) {
            if (j.framing && (size_t)nBlocks * bs > (size_t)0x7FFFFFFF) return fail(c, KNZ_ERR_INVALID_PARAM, "batch of %d blocks exceeds the 2 GiB per-call limit (pass max_blocks)", nBlocks);
            return 0;
        }
        // a stream of k blocks decodes to at most min(out_cap, k block sizes) bytes
        u64 most = 0;
        for (int i = 0; i < tab->nItems; i++) most += std::min<u64>(tab->items[i].out_cap, (u64)sw[(size_t)i].count * bs);
        if (most > (u64)0x7FFFFFFF) return fail(c, KNZ_ERR_INVALID_PARAM, "the streams of this call decode to up to %llu bytes, more than the 2 GiB per-call limit: split the call", (unsigned long long)most);
        return 0;
    }

    // The workspace stride S and the ranges the batch is decoded in
    int plan()
    {
        // large enough for every valid preTransformLength of this chain
        // (many streams: no block can be longer than the largest room, so the workspaces are sized by that and not by the block size -- a
        // thousand files of 1 KiB in a stream format of 4 MiB blocks take megabytes, not gigabytes; a longer block fails either way, with
        // the code it gets below where its room is too small)
        unit = tab ? std::max(tab->maxUnit, 1u) : j.framing ? bs : j.rawLen;
        S = ((u64)seq_stride(ch, (int)unit) + 255) & ~255ull;      // (the whole chain sizes the buffers, as in the encoder: a UTF stage adds 8 KiB of room)
        if (tab && (u64)nBlocks * S > STREAMS_MAX_WORK) return fail(c, KNZ_ERR_INVALID_PARAM, "%d blocks with a longest block of %u bytes exceed the workspace limit of a call (blocks x longest block <= 2 GiB): split the call", nBlocks, unit);
        maxChunks = (int)((S + ENT_CHUNK - 1) / ENT_CHUNK);
        outStride = j.framing ? bs : 0;
        // Up to three ranges side by side (knob dec_parts / KNZ_DEC_PARTS, default 3, at least KNZ_DEC_PART_MIN = 2 blocks per range -- 7 blocks: decode
        // 4.42 -> 4.04 ms; 4 blocks: no difference --; chains with inverse stages only; not
        // while per-kernel timing is on, not for chains with a stage that has no lanes): the entropy decoders are chains with a few
        // waves per CU and the row ranking of the BWT inverse is latency as well -- they run under the other ranges' bandwidth-bound kernels instead
        // of in front of them. Measured (26 blocks of 8 MiB, 1 / 2 / 3 ranges): decode 9.96 / 9.76 / 9.63 ms on the stand-in, 10.49 / 10.17 / 9.86 on the
        // real files; entropy-only chains (configs 1, 2) lose 2-5 % to the extra launches and stay one range.
        const int want = dec_parts_knob().load(), least = dec_part_min_knob().load();
        if (realMask && !c->profiling && lanesOk && j.nHosted == 0 && want > 1) {
            lanes = want > 3 ? 3 : want;
            while (lanes > 1 && nBlocks < least * lanes) lanes--;
        }
        return 0;
    }

    // Range k of the batch's blocks through entropy decoder and inverse chain, on stream `sp` with the workspaces of lane k (one range: lane
    // -1, the whole batch, whose BWT inverse may be split into parts). The blocks are independent and the walk has left every block's
    // place in the stream in d_blocks, so a range is a smaller decode of its own: its entries of d_blocks, its part of the caller's output.
    // It leaves every block's verdict, length and checksum verdict in its entries of d_blocks. The BWTS inverse synchronises `sp` (XF).
    int range(int k, hipStream_t sp)
    {
        const bool realStages = realMask != 0;
        const int lane = lanes > 1 ? k : -1;
        int b0, nb;
        cut(nBlocks, lanes, k, &b0, &nb);
        DecBlock* blk = d_blocks + b0;
        // (many streams: the blocks' places and rooms come from the tables, `room` only has to differ from ~0)
        uint8_t* out = tab ? j.d_out : j.d_out + (size_t)b0 * outStride;
        const u64 room = tab ? 0 : (u64)j.outCap - (u64)b0 * outStride;
        const u64* offT = tab ? d_outOff + b0 : nullptr;
        const u64* roomT = tab ? d_room + b0 : nullptr;
        SeqWs w;
        if (int r = seq_alloc(c, nb, S, realStages, chain_scratch_u32(ch, false, nb, (u32)S), &w, lane, sp)) return r;
        const size_t nSlots = (size_t)nb * maxChunks;
        // entropy stage decodes into workspace A (or straight into the output when no transform applies)
        // with inverse stages the entropy decoder writes into the workspace (any valid preTransformLength fits);
        // the room in the caller's buffer is enforced where the last inverse stage gets its capacity
        launch_check_prelen(sp, blk, nb, realStages ? (u32)S : unit, realStages ? ~0ull : room, outStride, roomT);
        launch_seq_inv_entropy_dst(sp, w.a, blk, nb, out, outStride, w.A, S, w.d_entDst, realMask, unit, room, offT, roomT);
        if (int r = ch.ec->decode({ c, sp, lane, src, blk, nb, S, maxChunks, nSlots, j.framing, bsVersion, j.streamBlockSize ? j.streamBlockSize : bs,
                                    ch.ec->extra, w.d_entDst })) return r;
        // inverse transforms, last stage first (TransformSequence.hpp:197-224)
        if (realStages) {
            const u32 capFinal = std::min(bs, unit);
            const u32 blkLenModel = std::max(bs + 512u, bs + (bs >> 4));
            const u32 capMid = (u32)std::min<u64>(S, blkLenModel);
            // (the reference's buffer, which the stages that judge by capacity go by, is sized by the stream's block size whatever the workspaces here are)
            const u32 capModel = (u32)std::min<u64>(((u64)seq_stride(ch, (int)bs) + 255) & ~255ull, blkLenModel);
            for (int i = ch.n - 1; i >= 0; i--) {
                if (ch.xf[i] == nullptr) continue;
                launch_seq_inv_prepare(sp, w.a, blk, nb, i, out, outStride, w.A, w.B, S, capMid, capFinal, realMask, room, offT, roomT);
                XfStage st = xf_stage(w, nb, (u32)S, p->entropy_type);
                st.bsVersion = bsVersion;
                st.maxCap = std::max(capMid, capFinal);
                st.capModel = capModel;
                st.blockSize = j.streamBlockSize ? j.streamBlockSize : bs;
                if (int r = run_stage(c, sp, *ch.xf[i], false, st, lane)) return r;
                launch_seq_inv_commit(sp, w.a, blk, nb, i, ch.tok[i]);
            }
        }
        if (p->checksum_bits && j.framing && j.nHosted == 0) {
            u64* d_sums;
            if (int r = ws_get(c, lane_ws("sums", lane), sizeof(u64) * nb, (void**)&d_sums, sp)) return r;
            launch_verify_checksums(sp, blk, nb, p->checksum_bits, out, outStride, w.d_viewPtr, w.a.alen, d_sums, offT);
        }
        return 0;
    }

    // The verdict on the blocks [b0, b1) of one stream, by the rules of DecodingTask::run: 0 and their bytes, or the first block that fails
    // (*bad) with its code, or with KNZ_ERR_PROCESS_BLOCK where it is short and not the last
    int judge(size_t b0, size_t b1, u64* bytes, size_t* bad) const
    {
        *bytes = 0;
        for (size_t b = b0; b < b1; b++) {
            *bad = b;
            if (hb[b].error) return hb[b].error;
            if (j.framing && b + 1 < b1 && hb[b].preLen != bs) return KNZ_ERR_PROCESS_BLOCK;
            *bytes += hb[b].preLen;
        }
        return 0;
    }

    // The blocks read back and judged: every item by itself, or the one stream for the call. Synchronises the stream.
    int results()
    {
        hb.resize((size_t)nBlocks);
        HIPCHK(c, hipMemcpyAsync(hb.data(), d_blocks, sizeof(DecBlock) * (size_t)nBlocks, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        u64 bytes;
        size_t bad = 0;
        if (tab) {
            for (int i = 0; i < tab->nItems; i++) {
                knz_item& it = tab->items[i];
                if (it.error) continue;
                const size_t b0 = (size_t)sw[(size_t)i].first;
                it.error = judge(b0, b0 + sw[(size_t)i].count, &bytes, &bad);
                it.out_len = it.error ? 0 : bytes;
            }
            return 0;
        }
        if (judge(0, (size_t)nBlocks, &bytes, &bad)) {
            const DecBlock& k = hb[bad];
            const int no = (int)bad + 1;
            if (!k.error) return fail(c, KNZ_ERR_PROCESS_BLOCK, "block %d: short non-final block (%u bytes) not supported", no, k.preLen);
            // (the first failing block ends the call, so the variable is read once)
            if (getenv("KNZ_DEBUG_ERR")) fprintf(stderr, "DBG block %d error %d used %llu\n", (int)bad, k.error, (unsigned long long)k.usedBits);
            // (a call without framing reports a block that does not decode as a result, not as a failure)
            if (!j.framing) { res.rawDecoded = -1; res.usedBits = k.usedBits; return 0; }
            return fail(c, k.error, "block %d: decoding failed (code %d)", no, k.error);
        }
        res.outBytes = bytes;
        res.skipOut = hb[0].copyBlock ? 0xFFu : hb[0].skipFlags;
        res.sumOut = hb[0].checksum;
        res.rawDecoded = (int32_t)hb[0].preLen;
        res.usedBits = hb[0].usedBits;
        return 0;
    }

    int run()
    {
        if (int r = check()) return r;
        if (int r = walk()) return r;
        if (nBlocks == 0) return 0;
        if (int r = limits()) return r;
        if (int r = plan()) return r;
        if (int r = fork_join(c, s, lanes, false, [this](int k, hipStream_t sp) { return range(k, sp); })) return r;
        HIPCHK(c, hipGetLastError());
        return results();
    }
};

// (end_bit and blocks_done also of a batch that fails behind its walk)
int knz_hip_decode_blocks(knz_ctx* ctx, const knz_params* p, const uint8_t* d_in, uint64_t in_bits, uint64_t start_bit,
                          int64_t max_blocks, uint8_t* d_out, size_t out_cap, uint64_t* out_bytes, uint64_t* end_bit,
                          int64_t* blocks_done)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    DecJob j;
    j.p = p; j.d_in = d_in; j.inBits = in_bits; j.startBit = start_bit; j.maxBlocks = max_blocks; j.d_out = d_out; j.outCap = out_cap;
    DecResult res;
    const int r = Decoder(c, j, res).run();
    if (res.walked && end_bit) *end_bit = res.endBit;
    if (res.walked && blocks_done) *blocks_done = res.blocksDone;
    if (r == 0 && out_bytes) *out_bytes = res.outBytes;
    return r;
}

int knz_hip_decode_block_hosted(knz_ctx* ctx, const knz_params* p, int32_t host_stages, const uint8_t* d_in, uint64_t in_bits, uint64_t start_bit,
                                uint8_t* d_out, size_t out_cap, uint64_t* out_bytes, uint64_t* end_bit, uint32_t* skip_flags, uint64_t* checksum, int32_t* done)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    DecJob j;
    j.p = p; j.d_in = d_in; j.inBits = in_bits; j.startBit = start_bit; j.maxBlocks = 1; j.d_out = d_out; j.outCap = out_cap; j.nHosted = host_stages;
    DecResult res;
    const int r = Decoder(c, j, res).run();
    if (res.walked && end_bit) *end_bit = res.endBit;
    if (r == 0 && out_bytes) *out_bytes = res.outBytes;
    if (skip_flags) *skip_flags = res.skipOut;
    if (checksum) *checksum = res.sumOut;
    if (done) *done = (int32_t)res.blocksDone;
    return r;
}

// ------------------------------------------------------------------------------------------------
// many streams in one call
// ------------------------------------------------------------------------------------------------
static size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

size_t knz_hip_encode_streams_bound(const knz_params* p, const knz_item* items, size_t n_items)
{
    size_t bound = 16;
    for (size_t i = 0; i < n_items; i++) bound += round16(knz_hip_encode_bound(p, (size_t)items[i].in_len) + ((size_t)items[i].prologue_bits + 7) / 8);
    return bound;
}

static int streams_block_size(Ctx* c, const knz_params* p, size_t nItems)
{
    const u32 bs = (u32)p->block_size;
    if (bs < 1024 || bs > (1u << 30) || (bs & 15)) return fail(c, KNZ_ERR_INVALID_PARAM, "invalid block size %u", bs);
    if (nItems > (size_t)KNZ_STREAMS_MAX_ITEMS) return fail(c, KNZ_ERR_INVALID_PARAM, "too many streams in one batch (%zu, at most %d)", nItems, KNZ_STREAMS_MAX_ITEMS);
    return 0;
}

int knz_hip_encode_streams(knz_ctx* ctx, const knz_params* p, const uint8_t* d_in, knz_item* items, size_t n_items, const uint8_t* prologues,
                           int finish, uint8_t* d_out, size_t out_cap, uint64_t* out_bytes)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    if (out_bytes) *out_bytes = 0;
    if (items == nullptr && n_items) return fail(c, KNZ_ERR_INVALID_PARAM, "no items");
    if (int r = streams_block_size(c, p, n_items)) return r;
    Chain ch;
    if (int r = parse_chain(c, p, 0, true, &ch)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const u32 bs = (u32)p->block_size;
    EncTab tab;
    tab.nItems = (int)n_items;
    tab.first.resize(n_items + 1);
    size_t total = 0, nBlocks = 0, proBytes = 0;
    for (size_t i = 0; i < n_items; i++) {
        const knz_item& it = items[i];
        if (it.in_off & 15) return fail(c, KNZ_ERR_INVALID_PARAM, "stream %zu: in_off %llu is no multiple of 16", i, (unsigned long long)it.in_off);
        if (((size_t)it.prologue_bits + 7) / 8 > 200) return fail(c, KNZ_ERR_INVALID_PARAM, "prologue too long");
        if (it.prologue_bits && prologues == nullptr) return fail(c, KNZ_ERR_INVALID_PARAM, "stream %zu: no prologue bytes", i);
        if (it.in_len > (u64)0x7FFFFFFF) return fail(c, KNZ_ERR_INVALID_PARAM, "batch of %llu bytes exceeds the 2 GiB per-call limit", (unsigned long long)it.in_len);
        tab.first[i] = (u32)nBlocks;
        total += (size_t)it.in_len;
        nBlocks += ((size_t)it.in_len + bs - 1) / bs;
        proBytes = std::max(proBytes, (size_t)it.prologue_off + ((size_t)it.prologue_bits + 7) / 8);
        if (total > (size_t)0x7FFFFFFF) return fail(c, KNZ_ERR_INVALID_PARAM, "batch of %zu bytes exceeds the 2 GiB per-call limit", total);
        if (nBlocks > (size_t)KNZ_STREAMS_MAX_BLOCKS) return fail(c, KNZ_ERR_INVALID_PARAM, "too many blocks in one batch (more than %d)", KNZ_STREAMS_MAX_BLOCKS);
    }
    tab.first[n_items] = (u32)nBlocks;
    tab.nBlocks = (int)nBlocks;
    const size_t need = knz_hip_encode_streams_bound(p, items, n_items);
    if (out_cap < need) return fail(c, KNZ_ERR_WRITE_FILE, "output buffer too small: need %zu have %zu", need, out_cap);

    // one upload: block offsets | streams | block lengths | the blocks' streams | prologue bytes; behind it the results and the scan's scratch
    const size_t oOff = 0, oSt = oOff + round16(8 * nBlocks), oLen = oSt + sizeof(StreamEnc) * (n_items + 1), oItem = oLen + round16(4 * nBlocks),
                 oPro = oItem + round16(4 * nBlocks), up = oPro + round16(proBytes + 8), oRes = up, oExcl = oRes + sizeof(StreamOut) * n_items;
    std::vector<u8> host(up, 0);
    u64* hOff = reinterpret_cast<u64*>(host.data() + oOff);
    StreamEnc* hSt = reinterpret_cast<StreamEnc*>(host.data() + oSt);
    u32* hLen = reinterpret_cast<u32*>(host.data() + oLen);
    u32* hItem = reinterpret_cast<u32*>(host.data() + oItem);
    for (size_t i = 0; i <= n_items; i++) {
        hSt[i].first = tab.first[i];
        if (i == n_items) break;
        const knz_item& it = items[i];
        hSt[i].prologueBits = it.prologue_bits; hSt[i].prologueOff = it.prologue_off;
        for (size_t k = 0, b = tab.first[i]; b < tab.first[i + 1]; k++, b++) {
            hOff[b] = it.in_off + (u64)k * bs;
            hLen[b] = (u32)std::min<u64>(bs, it.in_len - (u64)k * bs);
            hItem[b] = (u32)i;
            tab.maxLen = std::max(tab.maxLen, hLen[b]);
        }
    }
    if (proBytes) memcpy(host.data() + oPro, prologues, proBytes);
    tab.len.assign(hLen, hLen + nBlocks);
    u8* d_tab;
    hipStream_t s = c->stream;
    if (int r = ws_get(c, "streamTab", oExcl + 8 * (nBlocks + 1), (void**)&d_tab, s)) return r;
    HIPCHK(c, hipMemcpyAsync(d_tab, host.data(), up, hipMemcpyHostToDevice, s));
    tab.d_inOff = reinterpret_cast<const u64*>(d_tab + oOff); tab.d_st = reinterpret_cast<const StreamEnc*>(d_tab + oSt);
    tab.d_len = reinterpret_cast<const u32*>(d_tab + oLen); tab.d_itemOf = reinterpret_cast<const u32*>(d_tab + oItem);
    tab.d_pro = d_tab + oPro; tab.d_res = reinterpret_cast<StreamOut*>(d_tab + oRes); tab.d_excl = reinterpret_cast<u64*>(d_tab + oExcl);
    u64 bits = 0;
    EncJob j;
    j.p = p; j.d_in = d_in; j.n = total; j.finish = finish; j.d_out = d_out; j.outCap = out_cap; j.outBits = &bits; j.tab = &tab;
    const int r = Encoder(c, j).run();
    if (r) { hipStreamSynchronize(s); return r; }          // (`host` may still be on its way)
    for (size_t i = 0; i < n_items; i++) {
        items[i].out_off = tab.res[i].base;
        items[i].out_len = tab.res[i].bits;
        items[i].blocks = (int32_t)(tab.first[i + 1] - tab.first[i]);
        items[i].error = 0;
    }
    if (out_bytes) *out_bytes = bits / 8;
    return 0;
}

int knz_hip_decode_streams(knz_ctx* ctx, const knz_params* p, const uint8_t* d_in, knz_item* items, size_t n_items, uint8_t* d_out, size_t out_cap)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    if (items == nullptr && n_items) return fail(c, KNZ_ERR_INVALID_PARAM, "no items");
    if (int r = streams_block_size(c, p, n_items)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<StreamDec> sd(n_items);
    u64 reach = 0;
    u32 maxUnit = 0;
    for (size_t i = 0; i < n_items; i++) {
        knz_item& it = items[i];
        if ((it.in_off & 15) || (it.out_off & 15)) return fail(c, KNZ_ERR_INVALID_PARAM, "stream %zu: in_off and out_off must be multiples of 16", i);
        if (it.out_off > out_cap || it.out_cap > out_cap - it.out_off) return fail(c, KNZ_ERR_INVALID_PARAM, "stream %zu: its output range leaves the buffer", i);
        if (it.start_bit > it.in_len) return fail(c, KNZ_ERR_INVALID_PARAM, "stream %zu: start_bit behind the stream", i);
        sd[i].inOff = it.in_off; sd[i].inBits = it.in_len; sd[i].startBit = it.start_bit; sd[i].outOff = it.out_off; sd[i].outCap = it.out_cap;
        maxUnit = (u32)std::max<u64>(maxUnit, std::min<u64>(it.out_cap, (u64)p->block_size));
        reach = std::max(reach, 8 * it.in_off + it.in_len);
        it.out_len = 0; it.blocks = 0; it.error = 0;
    }
    if (n_items == 0) return 0;
    hipStream_t s = c->stream;
    u8* d_tab;
    const size_t oWalk = round16(sizeof(StreamDec) * n_items);
    if (int r = ws_get(c, "streamTab", oWalk + sizeof(StreamWalk) * (n_items + 1), (void**)&d_tab, s)) return r;
    HIPCHK(c, hipMemcpyAsync(d_tab, sd.data(), sizeof(StreamDec) * n_items, hipMemcpyHostToDevice, s));
    DecTab tab;
    tab.nItems = (int)n_items; tab.items = items; tab.maxUnit = maxUnit;
    tab.d_sd = reinterpret_cast<const StreamDec*>(d_tab); tab.d_walk = reinterpret_cast<StreamWalk*>(d_tab + oWalk);
    DecJob j;
    j.p = p; j.d_in = d_in; j.inBits = reach; j.d_out = d_out; j.outCap = out_cap; j.tab = &tab;
    DecResult res;
    const int r = Decoder(c, j, res).run();
    if (r) hipStreamSynchronize(s);
    return r;
}

// ------------------------------------------------------------------------------------------------
// many device-to-device copies in one launch (copy_many.hip)
// ------------------------------------------------------------------------------------------------
// the pinned staging of a call's table with room for `bytes`, free of the upload of the call before (whose kernel may still run)
static int tab_stage(Ctx* c, size_t bytes, u8** h)
{
    if (c->tabStageEv == nullptr) HIPCHK(c, hipEventCreateWithFlags(&c->tabStageEv, hipEventDisableTiming));
    HIPCHK(c, hipEventSynchronize(c->tabStageEv));
    if (c->tabStageCap < bytes) {
        if (c->tabStage) HIPCHK(c, hipHostFree(c->tabStage));
        c->tabStage = nullptr; c->tabStageCap = 0;
        const size_t want = bytes + (bytes >> 3) + 4096;
        HIPCHK(c, hipHostMalloc(&c->tabStage, want, hipHostMallocDefault));
        c->tabStageCap = want;
    }
    *h = reinterpret_cast<u8*>(c->tabStage);
    return 0;
}

// the staged table to the workspace `name` on the stream; the staging is free again once tabStageEv has passed
static int tab_upload(Ctx* c, const char* name, const u8* h, size_t bytes, hipStream_t s, u8** d_tab)
{
    if (int r = ws_get(c, name, bytes, (void**)d_tab, s)) return r;
    HIPCHK(c, hipMemcpyAsync(*d_tab, h, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(c->tabStageEv, s));
    return 0;
}

int knz_hip_copy_many(knz_ctx* ctx, const knz_copy* copies, size_t n)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    ProfInstall pi_(c);
    if (n == 0) return 0;
    if (copies == nullptr) return fail(c, KNZ_ERR_INVALID_PARAM, "no copies");
    if (n > (size_t)KNZ_COPY_MAX_COPIES) return fail(c, KNZ_ERR_INVALID_PARAM, "too many copies in one call (%zu, at most %d)", n, KNZ_COPY_MAX_COPIES);
    u64 tiles = 0;
    for (size_t i = 0; i < n; i++) {
        if (copies[i].len >> 32) return fail(c, KNZ_ERR_INVALID_PARAM, "copy %zu: %llu bytes, a copy takes fewer than 2^32", i, (unsigned long long)copies[i].len);
        tiles += copy_many_tiles(copies[i].dst, copies[i].len);
    }
    if (tiles >= (1ull << 31)) return fail(c, KNZ_ERR_INVALID_PARAM, "%llu tiles of %u bytes in one call, fewer than 2^31 are taken", (unsigned long long)tiles, copy_many_tile_bytes());
    if (tiles == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    // one upload: the copies | the exclusive prefix of their tile counts
    const size_t oFirst = sizeof(knz_copy) * n, bytes = oFirst + 4 * (n + 1);
    u8* h;
    if (int r = tab_stage(c, bytes, &h)) return r;
    memcpy(h, copies, oFirst);
    u32* first = reinterpret_cast<u32*>(h + oFirst);
    u32 at = 0;
    for (size_t i = 0; i < n; i++) { first[i] = at; at += (u32)copy_many_tiles(copies[i].dst, copies[i].len); }
    first[n] = at;
    u8* d_tab;
    if (int r = tab_upload(c, "copyTab", h, bytes, s, &d_tab)) return r;
    launch_copy_many(s, reinterpret_cast<const knz_copy*>(d_tab), reinterpret_cast<const u32*>(d_tab + oFirst), (u32)n, at);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// many buffers split into byte planes, or joined from them, in one launch (planes.hip)
// ------------------------------------------------------------------------------------------------
static int planes_many(knz_ctx* ctx, const knz_plane_copy* entries, size_t n, bool split)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    ProfInstall pi_(c);
    if (n == 0) return 0;
    if (entries == nullptr) return fail(c, KNZ_ERR_INVALID_PARAM, "no entries");
    if (n > (size_t)KNZ_COPY_MAX_COPIES) return fail(c, KNZ_ERR_INVALID_PARAM, "too many entries in one call (%zu, at most %d)", n, KNZ_COPY_MAX_COPIES);
    u64 tiles = 0;
    for (size_t i = 0; i < n; i++) {
        const knz_plane_copy& e = entries[i];
        if (e.elem != 1 && e.elem != 2 && e.elem != 4 && e.elem != 8) return fail(c, KNZ_ERR_INVALID_PARAM, "entry %zu: elements of %u bytes, 1, 2, 4 and 8 are taken", i, e.elem);
        if (e.reserved != 0) return fail(c, KNZ_ERR_INVALID_PARAM, "entry %zu: reserved is %u, not 0", i, e.reserved);
        if (e.len >> 32) return fail(c, KNZ_ERR_INVALID_PARAM, "entry %zu: %llu bytes, an entry takes fewer than 2^32", i, (unsigned long long)e.len);
        if (e.len % e.elem) return fail(c, KNZ_ERR_INVALID_PARAM, "entry %zu: %llu bytes are no multiple of its %u-byte elements", i, (unsigned long long)e.len, e.elem);
        tiles += planes_tiles(e.len);
    }
    if (tiles >= (1ull << 31)) return fail(c, KNZ_ERR_INVALID_PARAM, "%llu tiles of %u bytes in one call, fewer than 2^31 are taken", (unsigned long long)tiles, planes_tile_bytes());
    if (tiles == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    // one upload: the entries | the exclusive prefix of their tile counts
    const size_t oFirst = sizeof(knz_plane_copy) * n, bytes = oFirst + 4 * (n + 1);
    u8* h;
    if (int r = tab_stage(c, bytes, &h)) return r;
    memcpy(h, entries, oFirst);
    u32* first = reinterpret_cast<u32*>(h + oFirst);
    u32 at = 0;
    for (size_t i = 0; i < n; i++) { first[i] = at; at += (u32)planes_tiles(entries[i].len); }
    first[n] = at;
    u8* d_tab;
    if (int r = tab_upload(c, "copyTab", h, bytes, s, &d_tab)) return r;
    (split ? launch_split_many : launch_join_many)(s, reinterpret_cast<const knz_plane_copy*>(d_tab), reinterpret_cast<const u32*>(d_tab + oFirst), (u32)n, at);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int knz_hip_split_many(knz_ctx* ctx, const knz_plane_copy* entries, size_t n) { return planes_many(ctx, entries, n, true); }
int knz_hip_join_many(knz_ctx* ctx, const knz_plane_copy* entries, size_t n) { return planes_many(ctx, entries, n, false); }

// ------------------------------------------------------------------------------------------------
// per-stage (host buffers)
// ------------------------------------------------------------------------------------------------
int knz_hip_entropy_encode(knz_ctx* ctx, int entropy_type, const uint8_t* in, uint32_t n, uint8_t* out, size_t out_cap,
                           uint64_t* out_bits)
{
    return knz_hip_entropy_encode_bs(ctx, entropy_type, 0, in, n, out, out_cap, out_bits);
}

int knz_hip_entropy_encode_bs(knz_ctx* ctx, int entropy_type, uint32_t stream_block_size, const uint8_t* in, uint32_t n, uint8_t* out, size_t out_cap,
                              uint64_t* out_bits)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    if (stream_block_size > (1u << 30)) return fail(c, KNZ_ERR_INVALID_PARAM, "invalid block size %u", stream_block_size);
    if (n == 0) { *out_bits = 0; return 0; }
    knz_params p; memset(&p, 0, sizeof(p));
    p.entropy_type = entropy_type; p.block_size = (int32_t)((n + 15) & ~15u); p.transform_type = 0;
    u8 *d_in, *d_out;
    const size_t cap = knz_hip_encode_bound(&p, n);
    if (int r = ws_get(c, "stageIn", (size_t)n + 64, (void**)&d_in, c->stream)) return r;
    if (int r = ws_get(c, "stageOut", cap, (void**)&d_out, c->stream)) return r;
    HIPCHK(c, hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, c->stream));
    u64 bits = 0;
    EncJob j;
    j.p = &p; j.d_in = d_in; j.n = n; j.framing = 0; j.d_out = d_out; j.outCap = cap; j.outBits = &bits; j.streamBlockSize = stream_block_size;
    int r = Encoder(c, j).run();
    if (r == KNZ_ERR_WRITE_FILE && ec_info(entropy_type)->twoTier) {         // (an id without a row has failed in parse_chain, with another code)
        // the bound of the binary coders is their first tier (knz_hip_encode_bound): the second holds whatever the format can write
        const size_t cap2 = cap + 32 * (size_t)n;
        if (int r2 = ws_get(c, "stageOut", cap2, (void**)&d_out, c->stream)) return r2;
        j.d_out = d_out; j.outCap = cap2;
        r = Encoder(c, j).run();
    }
    if (r) return r;
    const size_t bytes = (size_t)((bits + 7) >> 3);
    if (bytes > out_cap) return fail(c, KNZ_ERR_WRITE_FILE, "output buffer too small");
    HIPCHK(c, hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out_bits = bits;
    return 0;
}

int knz_hip_entropy_decode(knz_ctx* ctx, int entropy_type, const uint8_t* in, uint64_t in_bits, uint64_t start_bit,
                           uint8_t* out, uint32_t n, int32_t* decoded, uint64_t* used_bits)
{
    return knz_hip_entropy_decode_v(ctx, entropy_type, 0, in, in_bits, start_bit, out, n, decoded, used_bits);
}

int knz_hip_entropy_decode_v(knz_ctx* ctx, int entropy_type, int bs_version, const uint8_t* in, uint64_t in_bits, uint64_t start_bit,
                             uint8_t* out, uint32_t n, int32_t* decoded, uint64_t* used_bits)
{
    return knz_hip_entropy_decode_bs(ctx, entropy_type, bs_version, 0, in, in_bits, start_bit, out, n, decoded, used_bits);
}

int knz_hip_entropy_decode_bs(knz_ctx* ctx, int entropy_type, int bs_version, uint32_t stream_block_size, const uint8_t* in, uint64_t in_bits,
                              uint64_t start_bit, uint8_t* out, uint32_t n, int32_t* decoded, uint64_t* used_bits)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    if (stream_block_size > (1u << 30)) return fail(c, KNZ_ERR_INVALID_PARAM, "invalid block size %u", stream_block_size);
    if (bs_version < 0 || bs_version > 6) return fail(c, KNZ_ERR_STREAM_VERSION, "cannot read bitstream version %d", bs_version);   // (as knz_hip_transform_inverse_v)
    if (n == 0) { *decoded = 0; if (used_bits) *used_bits = 0; return 0; }
    knz_params p; memset(&p, 0, sizeof(p));
    p.entropy_type = entropy_type; p.block_size = (int32_t)((n + 15) & ~15u); p.bs_version = bs_version;
    const size_t inBytes = (size_t)((in_bits + 7) >> 3);
    u8 *d_in, *d_out;
    if (int r = ws_get(c, "stageIn", inBytes + 64, (void**)&d_in, c->stream)) return r;
    if (int r = ws_get(c, "stageOut", (size_t)n + 64, (void**)&d_out, c->stream)) return r;
    HIPCHK(c, hipMemcpyAsync(d_in, in, inBytes, hipMemcpyHostToDevice, c->stream));
    DecJob j;
    j.p = &p; j.d_in = d_in; j.inBits = in_bits; j.startBit = start_bit; j.maxBlocks = 1; j.framing = 0; j.rawLen = n; j.d_out = d_out; j.outCap = n;
    j.streamBlockSize = stream_block_size;
    DecResult res;
    if (int r = Decoder(c, j, res).run()) return r;
    *decoded = res.rawDecoded;
    if (used_bits) *used_bits = res.usedBits;
    if (*decoded == (int32_t)n) {
        HIPCHK(c, hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

int knz_hip_tpaq_params(uint32_t stream_block_size, uint32_t block_len, int extra, uint32_t sizes[6])
{
    if (sizes == nullptr || (extra != 0 && extra != 1)) return KNZ_ERR_INVALID_PARAM;
    const TpaqSizes z = tpaq_params(stream_block_size, block_len, extra);
    sizes[0] = z.states; sizes[1] = z.mixers; sizes[2] = z.hash; sizes[3] = z.buffer; sizes[4] = z.sse0; sizes[5] = z.sse1;
    return 0;
}

int knz_hip_range_divide(knz_ctx* ctx, const uint64_t* d, const uint64_t* r, uint32_t n, uint32_t* q)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    u64 *d_d, *d_r; u32* d_q;
    if (int rc = ws_get(c, "stageIn", 16 * (size_t)n + 64, (void**)&d_d, c->stream)) return rc;
    if (int rc = ws_get(c, "stageOut", 4 * (size_t)n + 64, (void**)&d_q, c->stream)) return rc;
    d_r = d_d + n;
    HIPCHK(c, hipMemcpyAsync(d_d, d, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_r, r, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    launch_range_div_probe(c->stream, d_d, d_r, n, d_q);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(q, d_q, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int knz_hip_prims_info(uint32_t out[4])
{
    if (out == nullptr) return KNZ_ERR_INVALID_PARAM;
    prims_probe_info(out);
    return 0;
}

int knz_hip_prims_scan(knz_ctx* ctx, int op, const uint32_t* d_in, uint32_t* d_out, size_t n_max, const uint32_t* d_n, uint32_t* d_total)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    HIPCHK(c, hipSetDevice(c->device));
    char msg[256] = { 0 };
    const int r = prims_probe_scan(c->stream, op, d_in, d_out, n_max, d_n, d_total, msg, sizeof(msg));
    return r ? fail(c, r, "knz_hip_prims_scan: %s", msg) : 0;
}

int knz_hip_prims_sort(knz_ctx* ctx, int key_bytes, int has_val, int keep, int one_read, const void* d_keys, const uint32_t* d_vals,
                       const uint32_t* d_seg_base, int n_seg, size_t max_seg_len, int lo_bit, int hi_bit, void* d_keys_out, uint32_t* d_vals_out)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    CTX_LOCK(c);
    HIPCHK(c, hipSetDevice(c->device));
    char msg[256] = { 0 };
    const int r = prims_probe_sort(c->stream, key_bytes, has_val, keep, one_read, d_keys, d_vals, d_seg_base, n_seg, max_seg_len, lo_bit, hi_bit,
                                   d_keys_out, d_vals_out, msg, sizeof(msg));
    return r ? fail(c, r, "knz_hip_prims_sort: %s", msg) : 0;
}

static int transform_host(Ctx* c, int t, int forward, const uint8_t* in, int32_t n, uint8_t* out, int32_t dstCap, int etype,
                          int32_t* outLen, int32_t* ok, int bsVersion = 6, int32_t* dataType = nullptr, u32 streamBlockSize = 0)
{
    CTX_LOCK(c);
    ProfInstall pi_(c);
    *outLen = 0; *ok = 0;
    const XfInfo* x = xf_info(t);
    if (x == nullptr) return unsupported(c, t);
    if (n < 0 || dstCap < 0) return fail(c, KNZ_ERR_INVALID_PARAM, "negative size");
    if (n == 0) { *ok = 1; return 0; }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const u32 maxLen = (u32)std::max(n, dstCap) + 2048;
    SeqWs w;
    if (int r = seq_alloc(c, 1, maxLen, false, scratch_u32(forward ? x->fwd : x->inv, 1, maxLen), &w, -1, s)) return r;
    u8 *d_in, *d_out;
    if (int r = ws_get(c, "stageIn", (size_t)n + 64, (void**)&d_in, s)) return r;
    if (int r = ws_get(c, "stageOut", (size_t)maxLen + 64, (void**)&d_out, s)) return r;
    HIPCHK(c, hipMemcpyAsync(d_in, in, (size_t)n, hipMemcpyHostToDevice, s));
    struct { const u8* src; u8* dst; u32 len; u32 cap; } h;
    h.src = d_in; h.dst = d_out; h.len = (u32)n; h.cap = (u32)dstCap;
    HIPCHK(c, hipMemcpyAsync(w.a.src, &h.src, 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(w.a.dst, &h.dst, 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(w.a.alen, &h.len, 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(w.a.cap, &h.cap, 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(w.a.ok, 0, 1, s));
    HIPCHK(c, hipMemsetAsync(w.a.newLen, 0, 4, s));
    XfStage st = xf_stage(w, 1, (u32)n, etype);
    st.maxCap = (u32)dstCap;
    st.bsVersion = bsVersion;
    st.blockSize = streamBlockSize;
    u8 hdt = 0;
    if (dataType) {
        if (*dataType < 0 || *dataType > 9) return fail(c, KNZ_ERR_INVALID_PARAM, "data type %d out of range", *dataType);
        hdt = (u8)*dataType;
        HIPCHK(c, hipMemcpyAsync(w.a.dtype, &hdt, 1, hipMemcpyHostToDevice, s));
        st.dtype = w.a.dtype;
    }
    if (int r = run_stage(c, s, *x, forward != 0, st)) return r;
    HIPCHK(c, hipGetLastError());
    u8 hok = 0; u32 hlen = 0;
    HIPCHK(c, hipMemcpyAsync(&hok, w.a.ok, 1, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&hlen, w.a.newLen, 4, hipMemcpyDeviceToHost, s));
    if (dataType) HIPCHK(c, hipMemcpyAsync(&hdt, w.a.dtype, 1, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (dataType) *dataType = hdt;
    *ok = hok;
    if (hok) {
        *outLen = (int32_t)hlen;
        HIPCHK(c, hipMemcpyAsync(out, d_out, hlen, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    return 0;
}

int knz_hip_transform_supported(int transform_type) { return xf_info(transform_type) != nullptr ? 1 : 0; }

int knz_hip_transform_forward(knz_ctx* ctx, int transform_type, const uint8_t* in, int32_t n, uint8_t* out, int32_t dst_cap,
                              int entropy_type, int32_t* out_len, int32_t* ok)
{
    return transform_host(reinterpret_cast<Ctx*>(ctx), transform_type, 1, in, n, out, dst_cap, entropy_type, out_len, ok);
}

int knz_hip_transform_forward_dt(knz_ctx* ctx, int transform_type, const uint8_t* in, int32_t n, uint8_t* out, int32_t dst_cap,
                                 int entropy_type, int32_t* data_type, int32_t* out_len, int32_t* ok)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!data_type) return fail(c, KNZ_ERR_INVALID_PARAM, "no data type");
    return transform_host(c, transform_type, 1, in, n, out, dst_cap, entropy_type, out_len, ok, 6, data_type);
}

int knz_hip_transform_inverse(knz_ctx* ctx, int transform_type, const uint8_t* in, int32_t n, uint8_t* out, int32_t dst_cap,
                              int32_t* out_len, int32_t* ok)
{
    return transform_host(reinterpret_cast<Ctx*>(ctx), transform_type, 0, in, n, out, dst_cap, -1, out_len, ok);
}

int knz_hip_transform_inverse_v(knz_ctx* ctx, int transform_type, int bs_version, const uint8_t* in, int32_t n, uint8_t* out,
                                int32_t dst_cap, int32_t* out_len, int32_t* ok)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    const int v = (bs_version == 0) ? 6 : bs_version;
    if (v < 0 || v > 6) return fail(c, KNZ_ERR_STREAM_VERSION, "cannot read bitstream version %d", v);
    return transform_host(c, transform_type, 0, in, n, out, dst_cap, -1, out_len, ok, v);
}

int knz_hip_transform_forward_bs(knz_ctx* ctx, int transform_type, uint32_t stream_block_size, const uint8_t* in, int32_t n, uint8_t* out,
                                 int32_t dst_cap, int entropy_type, int32_t* data_type, int32_t* out_len, int32_t* ok)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!data_type) return fail(c, KNZ_ERR_INVALID_PARAM, "no data type");
    return transform_host(c, transform_type, 1, in, n, out, dst_cap, entropy_type, out_len, ok, 6, data_type, stream_block_size);
}

int knz_hip_transform_inverse_bs(knz_ctx* ctx, int transform_type, int bs_version, uint32_t stream_block_size, int entropy_type,
                                 const uint8_t* in, int32_t n, uint8_t* out, int32_t dst_cap, int32_t* out_len, int32_t* ok)
{
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    const int v = (bs_version == 0) ? 6 : bs_version;
    if (v < 0 || v > 6) return fail(c, KNZ_ERR_STREAM_VERSION, "cannot read bitstream version %d", v);
    return transform_host(c, transform_type, 0, in, n, out, dst_cap, entropy_type, out_len, ok, v, nullptr, stream_block_size);
}

}  // extern "C"
