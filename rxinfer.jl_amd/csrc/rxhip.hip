// rxhip.hip — host runtime and C ABI of librxhip (see include/rxhip.h).
//
// One engine handle = one batch of factor graphs lowered to a static device schedule:
// device buffers, per-model constant tables, one HIP stream, optional HIP-event profiling.
// No CPU fallback: if no HIP device is visible rxhip_lgssm_create fails with
// RXHIP_ERR_NO_DEVICE (the parity tests must exercise the kernels, never a host path).
#include "../../include/rxhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <set>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "launch_tables.hpp"
#include "gseq_kernels.hpp"
#include "drift_kernels.hpp"
#include "generic_kernels.hpp"
#include "engine.hpp"
#include "graph_lowering.hpp"   // (rxhip_lower::last_error: the thread-local text behind rxhip_lowering_error, for refusals that return no handle)
#include "model_envelope.hpp"

using namespace rxhip;
using plan::ScheduleHooks;

// The kernels templated on a dimension live in translation units of their own (launch_tables.hpp: tu_lgssm.hip per state dimension,
// tu_dense.hip per MFMA tile count); this file reaches them through LgssmVtbl / DenseVtbl.

// RXHIP_TRACE=1: stage timings of engine creation on stderr (measurement aid, off by default)
#include <chrono>
// Stages of an engine's creation (rxhip_get_create_stages): host arithmetic on model tables, device kernels that build tables
// (host time until they have been enqueued or — where the status is needed — finished), uploads, device memory allocation.
enum { STAGE_TABLES_HOST = 0, STAGE_TABLES_DEVICE, STAGE_UPLOAD, STAGE_ALLOC, STAGE_COUNT };
struct StageTrace {
    bool on;
    double* acc;   // the engine's stage_ms[STAGE_COUNT], or null
    std::chrono::steady_clock::time_point t0;
    explicit StageTrace(double* acc_ = nullptr) : on(std::getenv("RXHIP_TRACE") != nullptr), acc(acc_), t0(std::chrono::steady_clock::now()) {}
    void mark(const char* what, int stage = -1) {
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        if (acc && stage >= 0) acc[stage] += ms;
        if (on) std::fprintf(stderr, "[rxhip] %-28s %8.3f ms\n", what, ms);
        t0 = t1;
    }
};

static const std::vector<LgssmVtbl>& vtbls() {
    // every state dimension 1..4 with every observation dimension 1..4 (the reference is dimension-generic; d = 5 … 64 takes the MFMA
    // path with any dy ≤ 64).  Filling the tables launches nothing: a unit's code object is loaded with its first kernel.
    static const std::vector<LgssmVtbl> t = [] {
        std::vector<LgssmVtbl> v(16);
        lgssm_vtbls_d1(&v[0]);
        lgssm_vtbls_d2(&v[4]);
        lgssm_vtbls_d3(&v[8]);
        lgssm_vtbls_d4(&v[12]);
        return v;
    }();
    return t;
}
static const LgssmVtbl* find_vtbl(int d, int dy) {
    for (const auto& v : vtbls())
        if (v.d == d && v.dy == dy) return &v;
    return nullptr;
}

// ------------------------------------------------------------------------------------------
// layout helpers on device
__global__ void k_transpose_rows(const double* __restrict__ in, double* __restrict__ out, long long n_outer_in,
                                 long long n_inner_in, int k) {
    // in: [n_outer_in][n_inner_in][k]  ->  out: [n_inner_in][n_outer_in][k]
    const long long total = n_outer_in * n_inner_in * k;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (long long)gridDim.x * blockDim.x) {
        const long long e = g % k;
        const long long r = g / k;
        const long long o = r % n_outer_in;  // output is contiguous in (inner, outer, k): index by output
        const long long i = r / n_outer_in;
        out[g] = in[(o * n_inner_in + i) * k + e];
    }
}


// x[t][c][k] += sign · off[t][k]: known inputs (rxhip_lgssm_desc.state_offset / obs_offset) enter and leave the sweep as shifts
__global__ void k_shift_rows(double* __restrict__ x, const double* __restrict__ off, long long rows, long long n_chains, int k, double sign,
                             int per_chain = 0) {  // per_chain: `off` has the shape of x
    const long long total = rows * n_chains * k;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const long long t = g / (n_chains * k);
        x[g] += sign * (per_chain ? off[g] : off[t * k + g % k]);
    }
}
// out[i][t][k] = in[t][chains[i]][k]: posteriors of a few chains, chain-major (what `infer` returns for ONE chain)
__global__ void k_gather_chains(const double* __restrict__ in, double* __restrict__ out, const long long* __restrict__ chains,
                                long long n_sel, long long T, long long n_chains, int k) {
    const long long total = n_sel * T * k;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const long long e = g % k, r = g / k, t = r % T, i = r / T;
        out[g] = in[(t * n_chains + chains[i]) * k + e];
    }
}



// ---- idle-stream pool: on this runtime hipStreamCreate costs 1.5–9 ms and hipStreamDestroy ≈1.1 ms, which made
// engine construction + destruction ≈2.9 ms whatever the problem size.  Engine-owned streams are therefore recycled
// per device (drained before they are parked).  This is the library's only process-wide state; it is mutex-protected.
// rxhip_set_caching(0): a host that wants the ABI's "no global state" to the letter — nothing is parked, nothing is shared between handles, every pool below
// is bypassed (and emptied at the switch); the default (1) keeps them: they are what makes an engine-per-`infer(...)` host cheap.
#include <atomic>
static std::atomic<int> g_caching{1};
static bool caching_on() { return g_caching.load(std::memory_order_relaxed) != 0; }
struct StreamPool {
    std::mutex m;
    std::vector<std::pair<int, hipStream_t>> idle;
};
static StreamPool& stream_pool() {
    static StreamPool* p = new StreamPool;  // intentionally leaked: no destruction-order hazards at process exit
    return *p;
}
hipError_t rxhip::stream_acquire(int device, hipStream_t* out) {
    if (caching_on()) {
        StreamPool& sp = stream_pool();
        std::lock_guard<std::mutex> g(sp.m);
        for (size_t i = 0; i < sp.idle.size(); ++i)
            if (sp.idle[i].first == device) {
                *out = sp.idle[i].second;
                sp.idle.erase(sp.idle.begin() + (long)i);
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
// ---- what every creator, every run and every result getter shares (engine.hpp) ----
rxhip_status rxhip::new_handle(bool desc_ok, rxhip_engine** out, EngineKind kind) {
    if (!out) return RXHIP_ERR_BADARG;
    *out = nullptr;
    if (!desc_ok) return RXHIP_ERR_BADARG;
    rxhip_engine* e = new rxhip_engine();   // from here on every refusal carries a text (rxhip_last_error; the caller destroys the handle)
    *out = e;
    e->kind = kind;
    e->device = -1;
    return RXHIP_OK;
}
rxhip_status rxhip::count_devices(rxhip_engine* e, int* ndev) {
    *ndev = 0;
    if (hipGetDeviceCount(ndev) != hipSuccess || *ndev <= 0) return fail(e, RXHIP_ERR_NO_DEVICE, "no HIP device visible");
    return RXHIP_OK;
}
rxhip_status rxhip::finish_create(rxhip_engine* e, size_t chains, int fe_capacity) {
    HIPCHK(e, hipMalloc(&e->d_fe_chain, sizeof(double) * chains));
    HIPCHK(e, hipMemset(e->d_fe_chain, 0, sizeof(double) * chains));
    if (rxhip_status st = reserve(e, &e->fe_total_cap, fe_capacity, {{&e->d_fe_total, 1}})) return st;
    HIPCHK(e, hipMalloc(&e->d_status, sizeof(int)));
    HIPCHK(e, hipMemset(e->d_status, 0, sizeof(int)));
    return RXHIP_OK;
}
rxhip_status rxhip::open_device(rxhip_engine* e, DevGuard& guard, int device, void* stream, int ndev) {
    if (device >= 0) {
        if (device >= ndev) return fail(e, RXHIP_ERR_BADARG, "device %d out of range (%d visible)", device, ndev);
        e->device = device;
    } else
        HIPCHK(e, hipGetDevice(&e->device));
    HIPCHK(e, guard.set(e->device));
    if (stream) e->stream = (hipStream_t)stream;
    else {
        HIPCHK(e, stream_acquire(e->device, &e->stream));
        e->own_stream = true;
    }
    return RXHIP_OK;
}
rxhip_status rxhip::run_preamble(rxhip_engine* e, int32_t iterations, bool need_data) {
    if (iterations <= 0) return fail(e, RXHIP_ERR_BADARG, "run: iterations must be positive");
    if (need_data && !e->have_data) return fail(e, RXHIP_ERR_STATE, "run: no observations (call rxhip_set_data first)");
    return RXHIP_OK;
}
rxhip_status rxhip::reserve(rxhip_engine* e, int* cap, int iterations, std::initializer_list<IterBuf> bufs) {
    if (iterations <= *cap) return RXHIP_OK;
    if (e->stream) HIPCHK(e, hipStreamSynchronize(e->stream));
    *cap = 0;
    for (const IterBuf& b : bufs) {
        if (*b.p && !e->in_arena(*b.p)) HIPCHK(e, hipFree(*b.p));
        *b.p = nullptr;
    }
    for (const IterBuf& b : bufs) HIPCHK(e, hipMalloc(b.p, sizeof(double) * (size_t)iterations * b.per_iteration));
    *cap = iterations;
    return RXHIP_OK;
}
rxhip_status rxhip::check_observations(rxhip_engine* e, void (*launch)(rxhip_engine* e, long long n, unsigned nb), int bit, const char* message) {
    SET_DEVICE(e);
    const long long n = e->T * e->n_chains;
    launch(e, n, (unsigned)std::min<long long>((n + 255) / 256, 1024));
    HIPCHK(e, hipGetLastError());
    int st = 0;
    HIPCHK(e, hipMemcpyAsync(&st, e->d_status, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (st & bit) {
        HIPCHK(e, hipMemset(e->d_status, 0, sizeof(int)));
        e->have_data = false;
        return fail(e, RXHIP_ERR_BADARG, "%s", message);
    }
    return RXHIP_OK;
}
rxhip_status rxhip::results_ready(rxhip_engine* e, const char* name, bool wants_fe) {
    if (!e->ran) return fail(e, RXHIP_ERR_STATE, "%s: no run yet", name);
    if (wants_fe && !e->last_want_fe) return fail(e, RXHIP_ERR_STATE, "%s: free energy was not requested in the last run", name);
    return RXHIP_OK;
}
rxhip_status rxhip::open_results(rxhip_engine* e, DevGuard& guard, bool kind_ok, const char* name, bool wants_fe) {
    if (!kind_ok) return RXHIP_ERR_BADARG;
    if (rxhip_status st = results_ready(e, name, wants_fe)) return st;
    HIPCHK(e, guard.set(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return RXHIP_OK;
}
void rxhip::sum_chunk_partials(const double* part, size_t nchunk, size_t n, double* tot) {
    for (size_t q = 0; q < n; ++q) {
        double acc = part[q];
        for (size_t c = 1; c < nchunk; ++c) acc += part[c * n + q];
        tot[q] = acc;
    }
}
// Arenas up to 2 GB are parked the same way — hipFree of a multi-megabyte block costs ≈120–170 µs (more than a whole sweep of
// the reference's own benchmark sizes), hipMalloc + hipFree of the 1 GB of a d = 64, T = 10⁴ engine ≈40 ms.  At most 4 blocks /
// 4 GB are kept; rxhip_release_cached_memory() frees them.
struct ArenaPool {
    struct Blk { int device; char* p; size_t bytes; };
    std::mutex m;
    std::vector<Blk> idle;
    size_t total = 0;
};
static ArenaPool& arena_pool() {
    static ArenaPool* p = new ArenaPool;
    return *p;
}
// Pinned host staging blocks of the one-call path (rxhip_lgssm_infer): hipHostMalloc costs ≈0.1 ms, an `infer(...)` of the
// reference's own benchmark sizes builds an engine per call — so finished engines park their block here (at most 4, ≤ 8 MB each).
struct PinnedPool {
    struct Blk { double* p; size_t bytes; };
    std::mutex m;
    std::vector<Blk> idle;
};
static PinnedPool& pinned_pool() {
    static PinnedPool* p = new PinnedPool;
    return *p;
}
static double* pinned_acquire(size_t need, size_t* got) {
    if (caching_on()) {
        PinnedPool& pp = pinned_pool();
        std::lock_guard<std::mutex> g(pp.m);
        size_t best = pp.idle.size();   // the smallest block that fits (a 16 MB observation block is not spent on a status word)
        for (size_t i = 0; i < pp.idle.size(); ++i)
            if (pp.idle[i].bytes >= need && (best == pp.idle.size() || pp.idle[i].bytes < pp.idle[best].bytes)) best = i;
        if (best < pp.idle.size()) {
            double* p = pp.idle[best].p;
            *got = pp.idle[best].bytes;
            pp.idle.erase(pp.idle.begin() + (long)best);
            return p;
        }
    }
    double* p = nullptr;
    size_t bytes = need < ((size_t)64 << 10) ? ((size_t)64 << 10) : need;
    if (hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    *got = bytes;
    return p;
}
static void pinned_release(double* p, size_t bytes) {
    if (caching_on()) {
        PinnedPool& pp = pinned_pool();
        std::lock_guard<std::mutex> g(pp.m);
        if (pp.idle.size() < 6) {
            pp.idle.push_back({p, bytes});
            return;
        }
    }
    (void)hipHostFree(p);
}
// A pinned host block from the pool for the duration of a scope: what engine creation uploads (padded model matrices) and reads back
// (status words) goes through one — copies to / from PAGEABLE memory are staged or pinned by the runtime on the spot, which inside a
// process that holds tens of gigabytes of device memory was seen to cost 25 – 50 ms per engine (5 ms of builder kernels: DESIGN §6e).
struct PinnedTmp {
    double* p = nullptr;
    size_t bytes = 0;
    explicit PinnedTmp(size_t need) { if (need) p = pinned_acquire(need, &bytes); }
    PinnedTmp(const PinnedTmp&) = delete;
    PinnedTmp& operator=(const PinnedTmp&) = delete;
    ~PinnedTmp() { if (p) pinned_release(p, bytes); }
    double* detach() { double* q = p; p = nullptr; return q; }   // the caller keeps the block (and returns it to the pool itself)
};
static char* arena_acquire(int device, size_t need, size_t* got) {
    if (!caching_on()) return nullptr;
    ArenaPool& ap = arena_pool();
    std::lock_guard<std::mutex> g(ap.m);
    for (size_t i = 0; i < ap.idle.size(); ++i)
        if (ap.idle[i].device == device && ap.idle[i].bytes >= need && ap.idle[i].bytes <= 2 * need + (1 << 20)) {
            char* p = ap.idle[i].p;
            *got = ap.idle[i].bytes;
            ap.total -= ap.idle[i].bytes;
            ap.idle.erase(ap.idle.begin() + (long)i);
            return p;
        }
    return nullptr;
}
static void arena_release(int device, char* p, size_t bytes) {
    if (bytes > ((size_t)2 << 30) || !caching_on()) {
        (void)hipFree(p);
        return;
    }
    std::vector<char*> evict;
    {
        ArenaPool& ap = arena_pool();
        std::lock_guard<std::mutex> g(ap.m);
        while (!ap.idle.empty() && (ap.idle.size() >= 4 || ap.total + bytes > ((size_t)4 << 30))) {  // least recently parked first
            evict.push_back(ap.idle.front().p);
            ap.total -= ap.idle.front().bytes;
            ap.idle.erase(ap.idle.begin());
        }
        ap.idle.push_back({device, p, bytes});
        ap.total += bytes;
    }
    for (char* q : evict) (void)hipFree(q);
}
static void stream_release(int device, hipStream_t s) {
    (void)hipStreamSynchronize(s);
    StreamPool& sp = stream_pool();
    if (caching_on()) {
        std::lock_guard<std::mutex> g(sp.m);
        if (sp.idle.size() < 32) {
            sp.idle.emplace_back(device, s);
            return;
        }
    }
    (void)hipStreamDestroy(s);
}


// minimal "run this scope on device d, then go back" (the HIPCHK-aware DevGuard below needs an engine for its message)
struct DevGuardLite {
    int prev = -1;
    bool changed = false;
    explicit DevGuardLite(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DevGuardLite() { if (changed && prev >= 0) (void)hipSetDevice(prev); }
};

// The dynamic-LDS ceiling of a kernel is a per-device function attribute: set once per (kernel group, device), never per process
// (a host that drives several GPUs from one process would otherwise launch with the default 64 KB on every device but the first).
template <class F>
static void once_per_device(int group, int device, F set) {
    static std::mutex m;
    static std::set<std::pair<int, int>> done;
    std::lock_guard<std::mutex> g(m);
    if (done.insert({group, device}).second) {
        set();
        (void)hipGetLastError();
    }
}
// the same for a preparation that can fail (the dynamic-LDS ceilings of a kernel unit): remembered only once it has succeeded
template <class F>
static hipError_t once_per_device_checked(int group, int device, F set) {
    static std::mutex m;
    static std::set<std::pair<int, int>> done;
    std::lock_guard<std::mutex> g(m);
    if (done.count({group, device})) return hipSuccess;
    const hipError_t err = set();
    if (err == hipSuccess) done.insert({group, device});
    else (void)hipGetLastError();
    return err;
}

// ---- per-model device tables of the MFMA path, shared between engines ---------------------------------------------
// Constants, per-offset aggregation maps, boundary-scan maps and the boundary inverses depend on the model and the
// schedule only.  Building them costs ≈50 ms of host Riccati recursions + a 100 MB upload at d = 64 — two orders of
// magnitude more than a sweep — and `infer(...)` builds an engine per call, so engines of the same model (same bytes) share
// ONE read-only device copy: reference counted, a few idle copies kept (least recently used first out),
// rxhip_release_cached_memory() drops the idle ones.  Part of the library's mutex-protected process-wide state.
struct DenseTables {
    std::vector<unsigned char> key;
    int device = 0;
    char* block = nullptr;
    size_t bytes = 0;
    double *d_cst = nullptr, *d_tab = nullptr, *d_scanm = nullptr, *d_qtab = nullptr, *d_bnd = nullptr;
    int* d_canon = nullptr;
    int agg_oc = 1, agg_kc = 1, scan_sg = 1, scan_ng = 1;
    int refs = 0;
    unsigned long long last_use = 0;
};
struct DenseTablesPool {
    std::mutex m;
    std::vector<DenseTables*> all;
    unsigned long long clock = 0;
};
static DenseTablesPool& dense_tables_pool() {
    static DenseTablesPool* p = new DenseTablesPool;
    return *p;
}
static DenseTables* dense_tables_acquire(const std::vector<unsigned char>& key, int device) {
    if (!caching_on()) return nullptr;   // (every engine builds its own tables; they are freed with it: dense_tables_release)
    DenseTablesPool& tp = dense_tables_pool();
    std::lock_guard<std::mutex> g(tp.m);
    for (DenseTables* t : tp.all)
        if (t->device == device && t->key == key) {
            t->refs++;
            t->last_use = ++tp.clock;
            return t;
        }
    return nullptr;
}
static void dense_tables_insert(DenseTables* t) {
    DenseTablesPool& tp = dense_tables_pool();
    std::lock_guard<std::mutex> g(tp.m);
    t->refs = 1;
    t->last_use = ++tp.clock;
    tp.all.push_back(t);
}
// drop idle entries beyond `keep_idle` copies / `keep_bytes` bytes (least recently used first)
static void dense_tables_trim(size_t keep_idle, size_t keep_bytes) {
    std::vector<DenseTables*> victims;
    {
        DenseTablesPool& tp = dense_tables_pool();
        std::lock_guard<std::mutex> g(tp.m);
        for (;;) {
            size_t idle = 0, bytes = 0;
            DenseTables* lru = nullptr;
            for (DenseTables* t : tp.all)
                if (t->refs == 0) {
                    ++idle;
                    bytes += t->bytes;
                    if (!lru || t->last_use < lru->last_use) lru = t;
                }
            if (!lru || (idle <= keep_idle && bytes <= keep_bytes)) break;
            for (size_t i = 0; i < tp.all.size(); ++i)
                if (tp.all[i] == lru) { tp.all.erase(tp.all.begin() + (long)i); break; }
            victims.push_back(lru);
        }
    }
    for (DenseTables* t : victims) {
        DevGuardLite dg(t->device);
        (void)hipFree(t->block);
        delete t;
    }
}
static void dense_tables_release(DenseTables* t) {
    {
        DenseTablesPool& tp = dense_tables_pool();
        std::lock_guard<std::mutex> g(tp.m);
        t->refs--;
    }
    if (caching_on()) dense_tables_trim(4, (size_t)1 << 30);
    else dense_tables_trim(0, 0);
}

// ---- arena planning: register every buffer, then one hipMalloc, one upload of the table block, one memset ----
struct ArenaPlan {
    struct Item { void** pp; size_t bytes, off; const void* src; bool zero; bool edge; };
    std::vector<Item> up, zr, pl;  // uploaded tables | zero-initialised | plain
    template <class T> void upload(T** pp, const void* src, size_t bytes) { up.push_back({(void**)pp, bytes, 0, src, false, false}); }
    template <class T> void zeroed(T** pp, size_t bytes) { zr.push_back({(void**)pp, bytes, 0, nullptr, true, false}); }
    template <class T> void plain(T** pp, size_t bytes) { pl.push_back({(void**)pp, bytes, 0, nullptr, false, false}); }
    // the results of a run next to each other: the LAST zero-initialised item and the FIRST plain items (in the order of the calls) are adjacent
    // in the arena, so one device-to-host copy serves status word, marginals and free energies (rxhip_lgssm_infer)
    template <class T> void zeroed_last(T** pp, size_t bytes) { zr.push_back({(void**)pp, bytes, 0, nullptr, true, true}); }
    template <class T> void plain_first(T** pp, size_t bytes) { pl.push_back({(void**)pp, bytes, 0, nullptr, false, true}); }
    static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
};
static rxhip_status arena_commit(rxhip_engine* e, ArenaPlan& ap) {
    size_t off = 0;
    std::stable_partition(ap.zr.begin(), ap.zr.end(), [](const ArenaPlan::Item& it) { return !it.edge; });
    std::stable_partition(ap.pl.begin(), ap.pl.end(), [](const ArenaPlan::Item& it) { return it.edge; });
    for (auto* grp : {&ap.up, &ap.zr, &ap.pl})
        for (auto& it : *grp) { it.off = off; off += ArenaPlan::al(it.bytes ? it.bytes : 1); }
    const size_t up_end = ap.zr.empty() ? (ap.pl.empty() ? off : ap.pl.front().off) : ap.zr.front().off;
    const size_t zr_end = ap.pl.empty() ? off : ap.pl.front().off;
    size_t got = off;
    StageTrace tr(e->stage_ms);
    e->arena = arena_acquire(e->device, off, &got);
    if (!e->arena && hipMalloc(&e->arena, off) != hipSuccess) { e->arena = nullptr; return fail(e, RXHIP_ERR_HIP, "hipMalloc of %zu bytes failed", off); }
    e->arena_bytes = got;
    tr.mark("arena (pool or hipMalloc)", STAGE_ALLOC);
    for (auto* grp : {&ap.up, &ap.zr, &ap.pl})
        for (auto& it : *grp) *it.pp = e->arena + it.off;
    if (up_end) {
        // staged through a pinned block of the pool when it is small (the usual case: constants, priors, index tables — see PinnedTmp)
        std::vector<char> pageable;
        PinnedTmp pin(up_end <= ((size_t)4 << 20) ? up_end : 0);
        char* stage = pin.p && up_end <= ((size_t)4 << 20) ? reinterpret_cast<char*>(pin.p) : nullptr;
        if (!stage) { pageable.assign(up_end, 0); stage = pageable.data(); }
        else std::memset(stage, 0, up_end);
        for (auto& it : ap.up) std::memcpy(stage + it.off, it.src, it.bytes);
        if (hipMemcpyAsync(e->arena, stage, up_end, hipMemcpyHostToDevice, e->stream) != hipSuccess) return fail(e, RXHIP_ERR_HIP, "table upload failed");
        if (zr_end > up_end && hipMemsetAsync(e->arena + up_end, 0, zr_end - up_end, e->stream) != hipSuccess) return fail(e, RXHIP_ERR_HIP, "memset failed");
        if (pageable.empty() && !e->h_stage && e->h_mu.empty()) {   // (engines with known inputs rewrite uploaded regions with blocking copies later)
            // the pinned block stays with the engine until it is destroyed (behind a stream synchronisation): creation does not wait for the
            // upload — `infer(...)` of a small problem builds an engine per call, and this wait was a tenth of the call
            e->h_stage_bytes = pin.bytes;
            e->h_stage = pin.detach();
        } else if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(e, RXHIP_ERR_HIP, "table upload failed");  // `stage` dies here
    } else if (zr_end > up_end) {
        if (hipMemsetAsync(e->arena + up_end, 0, zr_end - up_end, e->stream) != hipSuccess) return fail(e, RXHIP_ERR_HIP, "memset failed");
    }
    tr.mark("arena upload + memset", STAGE_UPLOAD);
    return RXHIP_OK;
}

// ------------------------------------------------------------------------------------------
// host dense helpers for the per-model tables (generic n; off the hot path)
namespace host {
static bool chol_inv(int n, const double* A, double* out, double* logdet) {
    std::vector<double> L((size_t)n * n, 0.0), Li((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double s = A[j * n + j];
        for (int k = 0; k < j; ++k) s -= L[j * n + k] * L[j * n + k];
        if (!(s > 0.0)) return false;
        double ljj = std::sqrt(s);
        L[j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double t = 0.5 * (A[i * n + j] + A[j * n + i]);
            for (int k = 0; k < j; ++k) t -= L[i * n + k] * L[j * n + k];
            L[i * n + j] = t / ljj;
        }
    }
    if (logdet) {
        double ld = 0.0;
        for (int i = 0; i < n; ++i) ld += std::log(L[i * n + i]);
        *logdet = 2.0 * ld;
    }
    // Li = L⁻¹ row by row (row i of Li is e_i minus a combination of the rows above it), then A⁻¹ = Li'Li as a sum of
    // outer products of the rows of Li: every inner loop runs over contiguous memory (the tables of a d = 64, S = 250
    // engine need ≈750 of these inverses)
    for (int i = 0; i < n; ++i) {
        double* ri = &Li[(size_t)i * n];
        ri[i] = 1.0;
        for (int k = 0; k < i; ++k) {
            const double l = L[i * n + k];
            const double* rk = &Li[(size_t)k * n];
            for (int j = 0; j <= k; ++j) ri[j] -= l * rk[j];
        }
        const double inv = 1.0 / L[i * n + i];
        for (int j = 0; j <= i; ++j) ri[j] *= inv;
    }
    std::fill(out, out + (size_t)n * n, 0.0);
    for (int k = 0; k < n; ++k) {
        const double* rk = &Li[(size_t)k * n];
        for (int i = 0; i <= k; ++i) {
            const double a = rk[i];
            double* oi = out + (size_t)i * n;
            for (int j = 0; j <= i; ++j) oi[j] += a * rk[j];
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) out[(size_t)j * n + i] = out[(size_t)i * n + j];
    return true;
}
// Li = L⁻¹ with A = L L' (lower Cholesky factor): x'A⁻¹x = |Li x|² — the whitening maps of the free-energy residuals
static bool chol_linv(int n, const double* A, double* Li) {
    std::vector<double> L((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double s = A[j * n + j];
        for (int k = 0; k < j; ++k) s -= L[j * n + k] * L[j * n + k];
        if (!(s > 0.0)) return false;
        const double ljj = std::sqrt(s);
        L[j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double t = 0.5 * (A[i * n + j] + A[j * n + i]);
            for (int k = 0; k < j; ++k) t -= L[i * n + k] * L[j * n + k];
            L[i * n + j] = t / ljj;
        }
    }
    std::fill(Li, Li + (size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        double* ri = Li + (size_t)i * n;
        ri[i] = 1.0;
        for (int k = 0; k < i; ++k) {
            const double l = L[i * n + k];
            const double* rk = Li + (size_t)k * n;
            for (int j = 0; j <= k; ++j) ri[j] -= l * rk[j];
        }
        const double inv = 1.0 / L[i * n + i];
        for (int j = 0; j <= i; ++j) ri[j] *= inv;
    }
    return true;
}
// C[n×k] = A[n×m] B[m×k]   (row of C accumulated from rows of B: contiguous inner loops)
static void mm(int n, int m, int k, const double* A, const double* B, double* C) {
    for (int i = 0; i < n; ++i) {
        double* ci = C + (size_t)i * k;
        for (int j = 0; j < k; ++j) ci[j] = 0.0;
        for (int q = 0; q < m; ++q) {
            const double a = A[(size_t)i * m + q];
            const double* bq = B + (size_t)q * k;
            for (int j = 0; j < k; ++j) ci[j] += a * bq[j];
        }
    }
}
// C[n×k] = A[n×m] B'[k×m]   (dot products of rows, four partial sums)
static void mmT(int n, int m, int k, const double* A, const double* B, double* C) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < k; ++j) {
            const double *a = A + (size_t)i * m, *b = B + (size_t)j * m;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int q = 0;
            for (; q + 3 < m; q += 4) {
                s0 += a[q] * b[q];
                s1 += a[q + 1] * b[q + 1];
                s2 += a[q + 2] * b[q + 2];
                s3 += a[q + 3] * b[q + 3];
            }
            for (; q < m; ++q) s0 += a[q] * b[q];
            C[(size_t)i * k + j] = (s0 + s1) + (s2 + s3);
        }
}
// C[m×k] = A'[n×m] B[n×k]
static void mTm(int n, int m, int k, const double* A, const double* B, double* C) {
    std::fill(C, C + (size_t)m * k, 0.0);
    for (int q = 0; q < n; ++q) {
        const double* bq = B + (size_t)q * k;
        for (int i = 0; i < m; ++i) {
            const double a = A[(size_t)q * m + i];
            double* ci = C + (size_t)i * k;
            for (int j = 0; j < k; ++j) ci[j] += a * bq[j];
        }
    }
}
// two iterates of a recursion over symmetric positive (semi)definite matrices agree to rounding: every entry on the scale of its own row and column
static bool spd_same(int n, const double* x, const double* y, double tol) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double sc = std::sqrt(std::fabs(x[(size_t)i * n + i] * x[(size_t)j * n + j]));
            if (!(std::fabs(x[(size_t)i * n + j] - y[(size_t)i * n + j]) <= tol * sc)) return false;
        }
    return true;
}
static void pack_sym(int n, const double* A, double* out) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) out[sidx(i, j)] = 0.5 * (A[i * n + j] + A[j * n + i]);
}
}  // namespace host
bool rxhip::host_chol_inv(int n, const double* A, double* out, double* logdet) { return host::chol_inv(n, A, out, logdet); }

// Build constant block, gain tables and element matrices of one model.
struct HostAgg { std::vector<double> Pi, C, J, Ci, X, JJ; };
// host part of the one-pass schedule's tables (F0Layout, PosLayout, FeSegLayout) and the data-independent evidence terms
struct FusedTables { std::vector<double> ftab, pos, fseg; double fe_const = 0.0; };

// data-independent part of the boundary scan (see ScanLayout / DenseParams::scanm): per segment the maps that
// carry the means / weighted means across it, the covariance at its start and the backward precision at its end
// Flat tables, [S][d·d] each (one allocation per table: a chain cut into 250 short segments used to pay 1500 small allocations here).
static bool build_scan_matrices(int d, int S, const HostAgg& a0, const HostAgg& aLast, const double* Vf1, std::vector<double>& M1,
                                std::vector<double>& M2, std::vector<double>& Vb, std::vector<double>& N1, std::vector<double>& N2,
                                std::vector<double>& Lb) {
    const size_t MM = (size_t)d * d, n = (size_t)S * MM;
    M1.assign(n, 0.0); M2.assign(n, 0.0); Vb.assign(n, 0.0); N1.assign(n, 0.0); N2.assign(n, 0.0); Lb.assign(n, 0.0);
    std::vector<double> Vc(Vf1, Vf1 + MM), Vi(MM), W(MM), tt(MM), m1(MM), m2(MM), Vprev(MM, 0.0);
    auto at = [MM](std::vector<double>& t, int s) { return t.data() + (size_t)s * MM; };
    // Both recursions are Riccati maps of a time-invariant model: once an iterate reproduces its predecessor to rounding every later segment takes
    // the previous segment's maps — a chain cut into 250 short segments costs what its first few dozen do.  "To rounding" is decided ENTRY BY
    // ENTRY on each entry's own scale, |Δ_ij| ≤ RXHIP_TAB_SAME_TOL sqrt(x_ii x_jj) (host::spd_same): relative to the largest entry (rounds 2–4) the test was blind
    // to a slowly converging block whose units put it decades below another one (tests/test_fixed_point_adversarial_gpu.py).
    auto same = [d](const std::vector<double>& x, const std::vector<double>& y) { return host::spd_same(d, x.data(), y.data(), RXHIP_TAB_SAME_TOL); };
    bool conv = false;
    for (int s = 0; s < S; ++s) {
        std::memcpy(at(Vb, s), Vc.data(), sizeof(double) * MM);
        if (s == S - 1) break;
        if (!conv && s > 0 && same(Vc, Vprev)) conv = true;
        if (conv) {   // M1, M2 of the previous segment; Vc stays
            std::memcpy(at(M1, s), at(M1, s - 1), sizeof(double) * MM);
            std::memcpy(at(M2, s), at(M2, s - 1), sizeof(double) * MM);
            continue;
        }
        Vprev = Vc;
        if (!host::chol_inv(d, Vc.data(), Vi.data(), nullptr)) return false;
        for (size_t q = 0; q < MM; ++q) tt[q] = Vi[q] + a0.J[q];
        if (!host::chol_inv(d, tt.data(), W.data(), nullptr)) return false;
        host::mm(d, d, d, a0.Pi.data(), W.data(), m2.data());
        host::mm(d, d, d, m2.data(), Vi.data(), m1.data());
        host::mmT(d, d, d, m2.data(), a0.Pi.data(), tt.data());
        std::memcpy(at(M1, s), m1.data(), sizeof(double) * MM);
        std::memcpy(at(M2, s), m2.data(), sizeof(double) * MM);
        for (int a = 0; a < d; ++a)
            for (int b = 0; b <= a; ++b) {
                const double v = 0.5 * (tt[a * d + b] + tt[b * d + a]) + a0.C[a * d + b];
                Vc[a * d + b] = Vc[b * d + a] = v;
            }
    }
    std::vector<double> Lm(MM, 0.0), n1(MM), n2(MM), Lprev(MM, 0.0);
    conv = false;
    for (int s = S - 1; s >= 1; --s) {  // Lb[s] = Λβ(b_{s+1})
        const HostAgg& g = (s == S - 1) ? aLast : a0;
        std::memcpy(at(Lb, s), Lm.data(), sizeof(double) * MM);
        if (!conv && s < S - 2 && same(Lm, Lprev)) conv = true;   // (from the second full segment on: the last segment has its own element)
        if (conv) {
            std::memcpy(at(N1, s), at(N1, s + 1), sizeof(double) * MM);
            std::memcpy(at(N2, s), at(N2, s + 1), sizeof(double) * MM);
            continue;
        }
        Lprev = Lm;
        for (size_t q = 0; q < MM; ++q) tt[q] = g.Ci[q] + Lm[q];
        if (!host::chol_inv(d, tt.data(), W.data(), nullptr)) return false;
        host::mTm(d, d, d, g.X.data(), W.data(), n1.data());
        host::mm(d, d, d, n1.data(), Lm.data(), n2.data());
        host::mm(d, d, d, n1.data(), g.X.data(), tt.data());
        std::memcpy(at(N1, s), n1.data(), sizeof(double) * MM);
        std::memcpy(at(N2, s), n2.data(), sizeof(double) * MM);
        for (int a = 0; a < d; ++a)
            for (int b = 0; b <= a; ++b) {
                const double v = g.JJ[a * d + b] - 0.5 * (tt[a * d + b] + tt[b * d + a]);
                Lm[a * d + b] = Lm[b * d + a] = v;
            }
    }
    if (S > 0) std::memcpy(at(Lb, 0), Lm.data(), sizeof(double) * MM);
    return true;
}

static rxhip_status build_model_tables(rxhip_engine* e, int mdl, const rxhip_lgssm_desc* ds, double* cst,
                                       double* tab, double* agg, std::vector<double>* scan_out, FusedTables* fused = nullptr) {
    const LgssmVtbl& v = *e->vt;
    const int d = e->d, dy = e->dy;
    const double* A = ds->A + (size_t)mdl * d * d;
    const double* B = ds->B + (size_t)mdl * dy * d;
    const double* P = ds->P + (size_t)mdl * d * d;
    const double* Q = ds->Q + (size_t)mdl * dy * dy;
    const double* m0 = ds->m0 + (size_t)mdl * d;
    const double* V0 = ds->V0 + (size_t)mdl * d * d;
    std::vector<double> Qi(dy * dy), tmp(4 * (d + dy) * (d + dy)), G(d * dy), Lobs(d * d), HF(dy * d), V1(d * d),
        m1(d), scratch(d * d);
    double ldQ = 0.0;
    if (!host::chol_inv(dy, Q, Qi.data(), &ldQ))
        return fail(e, RXHIP_ERR_NOT_POSDEF, "model %d: observation noise Q is not positive definite", mdl);
    if (!host::chol_inv(d, P, scratch.data(), nullptr))
        return fail(e, RXHIP_ERR_NOT_POSDEF, "model %d: state noise P is not positive definite", mdl);
    host::mTm(dy, d, dy, B, Qi.data(), G.data());    // G = B' Qi  (d×dy)
    host::mm(d, dy, d, G.data(), B, Lobs.data());    // Lobs = B' Qi B
    host::mm(dy, d, d, B, A, HF.data());             // HF = B A
    if (e->ptt) {
        for (int i = 0; i < d; ++i) {
            double s = 0.0;
            for (int k = 0; k < d; ++k) s += A[i * d + k] * m0[k];
            m1[i] = s;
        }
        host::mm(d, d, d, A, V0, tmp.data());
        host::mmT(d, d, d, tmp.data(), A, V1.data());
        for (int i = 0; i < d * d; ++i) V1[i] += P[i];
    } else {
        for (int i = 0; i < d; ++i) m1[i] = m0[i];
        for (int i = 0; i < d * d; ++i) V1[i] = V0[i];
    }
    if (!host::chol_inv(d, V1.data(), scratch.data(), nullptr))
        return fail(e, RXHIP_ERR_NOT_POSDEF, "model %d: prior covariance is not positive definite", mdl);

    std::memset(cst, 0, sizeof(double) * v.cst_size);
    for (int i = 0; i < d * d; ++i) cst[v.oA + i] = A[i];
    host::pack_sym(d, P, cst + v.oP);
    host::pack_sym(d, Lobs.data(), cst + v.oLOBS);
    for (int i = 0; i < d * dy; ++i) cst[v.oG + i] = G[i];
    host::pack_sym(dy, Qi.data(), cst + v.oQI);
    cst[v.oC0] = dy * 1.8378770664093454835606594728112 + ldQ;
    for (int i = 0; i < d; ++i) cst[v.oM1 + i] = m1[i];
    host::pack_sym(d, V1.data(), cst + v.oV1);
    for (int i = 0; i < dy * d; ++i) cst[v.oHF + i] = HF[i];

    // gain tables: Kalman filter started from an exactly known state (V = 0)
    const long long L = e->sequential ? 0 : e->L;
    std::vector<double> V(d * d, 0.0), Pi(d * d, 0.0), J(d * d, 0.0), Vp(d * d), S(dy * dy), Si(dy * dy), K(d * dy),
        HFPi(dy * d), U(d * dy), t1(d * d + dy * d + d * dy), t2(d * d + dy * d + d * dy), Phi(d * d), Ci(d * d),
        X(d * d), JJ(d * d);
    for (int i = 0; i < d; ++i) Pi[i * d + i] = 1.0;
    std::memset(agg, 0, sizeof(double) * 2 * v.agg_size);
    HostAgg hagg[2];
    std::vector<double> ld_prefix;  // Σ_{k ≤ i} logdet S⁰_k
    if (fused) {
        fused->ftab.assign((size_t)L * v.f0_size, 0.0);
        fused->pos.assign((size_t)L * v.pos_size, 0.0);
        ld_prefix.assign((size_t)L + 1, 0.0);
    }
    for (long long i = 1; i <= L; ++i) {
        host::mm(d, d, d, A, V.data(), t1.data());
        host::mmT(d, d, d, t1.data(), A, Vp.data());
        for (int q = 0; q < d * d; ++q) Vp[q] += P[q];
        host::mm(dy, d, d, B, Vp.data(), t1.data());   // B Vp (dy×d)
        host::mmT(dy, d, dy, t1.data(), B, S.data());  // B Vp B'
        for (int q = 0; q < dy * dy; ++q) S[q] += Q[q];
        double ldS = 0.0;
        if (!host::chol_inv(dy, S.data(), Si.data(), &ldS))
            return fail(e, RXHIP_ERR_NOT_POSDEF, "model %d: innovation covariance not positive definite", mdl);
        host::mTm(dy, d, dy, t1.data(), Si.data(), K.data());       // K = (B Vp)' Si  (d×dy)
        host::mm(dy, d, d, HF.data(), Pi.data(), HFPi.data());      // HF Π_{i-1}
        host::mTm(dy, d, dy, HFPi.data(), Si.data(), U.data());     // U = (HF Π)' Si  (d×dy)
        host::mm(d, dy, d, U.data(), HFPi.data(), t2.data());       // (HFΠ)' Si (HFΠ)
        for (int q = 0; q < d * d; ++q) J[q] += t2[q];
        // V = Vp − K (B Vp)
        host::mm(d, dy, d, K.data(), t1.data(), t2.data());
        for (int a = 0; a < d; ++a)
            for (int b = 0; b <= a; ++b) {
                double s = 0.5 * ((Vp[a * d + b] - t2[a * d + b]) + (Vp[b * d + a] - t2[b * d + a]));
                V[a * d + b] = V[b * d + a] = s;
            }
        // Π = (A − K HF) Π
        host::mm(d, dy, d, K.data(), HF.data(), t2.data());
        for (int q = 0; q < d * d; ++q) Phi[q] = A[q] - t2[q];
        host::mm(d, d, d, Phi.data(), Pi.data(), t2.data());
        for (int q = 0; q < d * d; ++q) Pi[q] = t2[q];
        double* te = tab + (size_t)(i - 1) * v.tab_size;
        for (int q = 0; q < d * dy; ++q) {
            te[v.tK + q] = K[q];
            te[v.tU + q] = U[q];
        }
        if (fused) {
            double* fe = fused->ftab.data() + (size_t)(i - 1) * v.f0_size;
            for (int q = 0; q < d * dy; ++q) {
                fe[v.fK + q] = K[q];
                fe[v.fU + q] = U[q];
            }
            host::pack_sym(dy, Si.data(), fe + v.fSI);
            double* pe = fused->pos.data() + (size_t)(i - 1) * v.pos_size;
            for (int q = 0; q < d * d; ++q) pe[v.pPI + q] = Pi[q];
            host::pack_sym(d, J.data(), pe + v.pJ);
            host::pack_sym(d, V.data(), pe + v.pC);
            ld_prefix[(size_t)i] = ld_prefix[(size_t)i - 1] + ldS;
        }
        for (int which = 0; which < 2; ++which) {
            const long long want = which == 0 ? L : e->Llast;
            if (i != want) continue;
            double* ag = agg + (size_t)which * v.agg_size;
            if (!host::chol_inv(d, V.data(), Ci.data(), nullptr))
                return fail(e, RXHIP_ERR_NOT_POSDEF, "model %d: segment covariance not positive definite", mdl);
            host::mm(d, d, d, Ci.data(), Pi.data(), X.data());
            host::mTm(d, d, d, Pi.data(), X.data(), JJ.data());
            for (int q = 0; q < d * d; ++q) JJ[q] += J[q];
            for (int q = 0; q < d * d; ++q) {
                ag[v.aPI + q] = Pi[q];
                ag[v.aX + q] = X[q];
            }
            host::pack_sym(d, V.data(), ag + v.aC);
            host::pack_sym(d, J.data(), ag + v.aJ);
            host::pack_sym(d, Ci.data(), ag + v.aCI);
            host::pack_sym(d, JJ.data(), ag + v.aJJ);
            HostAgg& h = hagg[which];
            h.Pi = Pi; h.C = V; h.J = J; h.Ci = Ci; h.X = X; h.JJ = JJ;
            for (int a = 0; a < d; ++a)
                for (int b = 0; b < a; ++b) {
                    double sj = 0.5 * (h.J[a * d + b] + h.J[b * d + a]); h.J[a * d + b] = h.J[b * d + a] = sj;
                    double sq = 0.5 * (h.JJ[a * d + b] + h.JJ[b * d + a]); h.JJ[a * d + b] = h.JJ[b * d + a] = sq;
                }
        }
    }
    if (scan_out && e->S > 0) {
        // filtered covariance at t = 1: (V1⁻¹ + B'Q⁻¹B)⁻¹
        std::vector<double> V1i(d * d), Lf(d * d), Vf1(d * d);
        if (!host::chol_inv(d, V1.data(), V1i.data(), nullptr)) return fail(e, RXHIP_ERR_NOT_POSDEF, "prior covariance is not positive definite");
        for (int q = 0; q < d * d; ++q) Lf[q] = V1i[q] + Lobs[q];
        if (!host::chol_inv(d, Lf.data(), Vf1.data(), nullptr)) return fail(e, RXHIP_ERR_NOT_POSDEF, "first filtered precision not positive definite");
        std::vector<double> M1, M2, Vb, N1, N2, Lb;   // [S][d·d] each
        const size_t MMs = (size_t)d * d;
        if (!build_scan_matrices(d, e->S, hagg[0], hagg[1], Vf1.data(), M1, M2, Vb, N1, N2, Lb))
            return fail(e, RXHIP_ERR_NOT_POSDEF, "model %d: boundary scan matrix not positive definite", mdl);
        scan_out->assign((size_t)e->S * v.scan_size, 0.0);
        for (int s = 0; s < e->S; ++s) {
            double* t = scan_out->data() + (size_t)s * v.scan_size;
            for (int q = 0; q < d * d; ++q) { t[v.sM1 + q] = M1[s * MMs + q]; t[v.sM2 + q] = M2[s * MMs + q]; t[v.sN1 + q] = N1[s * MMs + q]; t[v.sN2 + q] = N2[s * MMs + q]; }
            host::pack_sym(d, Vb.data() + s * MMs, t + v.sVB);
            host::pack_sym(d, Lb.data() + s * MMs, t + v.sLB);
        }
        if (fused) {
            // per segment: −2 log p(y_seg | y_before) = [len·dy·log 2π + Σ logdet S⁰_i + logdet(I + V_s J)] + q0
            //                                           + m_s'A1 m_s − 2 η'A2 m_s − η'W η
            fused->fseg.assign((size_t)e->S * v.fs_size, 0.0);
            fused->fe_const = 0.0;
            std::vector<double> Vi(d * d), W(d * d), A2(d * d), A1(d * d), tt(d * d);
            for (int s = 0; s < e->S; ++s) {
                const HostAgg& g = (s == e->S - 1) ? hagg[1] : hagg[0];
                const long long len = (s == e->S - 1) ? e->Llast : L;
                double ldV = 0.0, ldT = 0.0;
                if (!host::chol_inv(d, Vb.data() + s * MMs, Vi.data(), &ldV)) return fail(e, RXHIP_ERR_NOT_POSDEF, "segment start covariance not positive definite");
                for (int q = 0; q < d * d; ++q) tt[q] = Vi[q] + g.J[q];
                if (!host::chol_inv(d, tt.data(), W.data(), &ldT)) return fail(e, RXHIP_ERR_NOT_POSDEF, "segment precision not positive definite");
                host::mm(d, d, d, W.data(), Vi.data(), A2.data());
                host::mm(d, d, d, g.J.data(), A2.data(), A1.data());
                double* f = fused->fseg.data() + (size_t)s * v.fs_size;
                host::pack_sym(d, A1.data(), f + v.fsA1);
                for (int q = 0; q < d * d; ++q) f[v.fsA2 + q] = A2[q];
                host::pack_sym(d, W.data(), f + v.fsW);
                fused->fe_const += (double)len * dy * 1.8378770664093454835606594728112 + ld_prefix[(size_t)len] + ldV + ldT;
            }
        }
    }
    return RXHIP_OK;
}


// ------------------------------------------------------------------------------------------
// dense path (d multiple of 16, ≤ 64): host-side per-model tables and launches
// any state dimension up to 64: the MFMA path runs on d rounded up to a multiple of 16, the extra dimensions are
// decoupled padding (A = 0, P = V0 = I, m0 = 0, B = 0: posterior N(0, I), no contribution to the free energy)
static bool dense_supported(int d, int dy) { return d >= 1 && d <= 64 && dy >= 1 && dy <= 64; }
static int dense_pad(int d) { return (d + 15) / 16 * 16; }

static const DenseVtbl* dense_vt(int nt) {
    switch (nt) {
        case 1: return dense_vtbl_nt1();
        case 2: return dense_vtbl_nt2();
        case 3: return dense_vtbl_nt3();
        default: return dense_vtbl_nt4();
    }
}
// free-energy residual terms of an information-form smoothing run: one workgroup per FR_STEPS steps, partial slots 2S…
static int fe_resid_blocks(long long T, int d, int dy) { const int st = fe_resid_steps(d, dy); return (int)((T + st - 1) / st); }
static long long mseg_resid_slots(long long T, int d, int dy, bool stepm, int models);
// passes > 1: per-step constants — one launch per model, each with its own partial slots, the columns of the other models masked
static long long mseg_resid_slots(long long T, int d, int dy, bool stepm, int models) {   // partial slots the residual kernel(s) write per chain
    if (stepm && models > FE_RESID_MAX_PASSES) return (T + FE_STEPS_BLOCK - 1) / FE_STEPS_BLOCK;
    return (long long)(stepm ? models : 1) * fe_resid_blocks(T, d, dy);
}
static void launch_fe_resid(const DenseParams& p, hipStream_t s, int passes = 1) { dense_vt(p.d / 16)->fe_resid(p, s, passes); }
#define DENSE_DISPATCH(nt, CALL) dense_vt(nt)->CALL
static int dense_tri(int nt) { return nt * (nt + 1) / 2 * 256; }
static int dense_rec(int nt) { return 3 * 16 * nt + 2 * 256 * nt * nt; }  // DenseCfg<NT>::REC

// Integer parameters of the MFMA schedule that depend on (L, S) only: K-chunks of the aggregation GEMM, groups of the two-level scan
static void dense_schedule_ints(rxhip_engine* e) {
    long long oc = (e->L + 11) / 12;
    if (oc < 1) oc = 1;
    e->agg_oc = (int)oc;
    e->agg_kc = (int)((e->L + oc - 1) / oc);
    const int n = e->S - 1;
    int sg = 1;
    while (sg * sg < n) ++sg;
    e->scan_sg = sg;
    e->scan_ng = n > 0 ? (n + sg - 1) / sg : 1;
}

static bool dense_tab_on_device(const rxhip_engine* e) {
    // d ≥ 32: below, the host recursions take well under a millisecond (and a 16×16 model padded into these kernels would not be faster)
    return e->nt >= 2 && e->dyk <= e->dpad && !e->hooks.host_tables;
}

// ---- `missing` observations on the MFMA path, parallel in time (dense_mseg_kernels.hpp) -------------------------------------
// Eligible engines: dense, allow_missing, ONE model, no per-step constants, dy ≤ padded d, at least two time steps.  They stay
// gseq engines for everything else (filtering runs, the step-wise filter, predictions, node-local joints run on the sequential
// kernels); smoothing runs take the time-parallel schedule unless RXHIP_GSEQ is set (the sequential schedule as the checker).
static rxhip_status mseg_setup(rxhip_engine* e, const rxhip_lgssm_desc* ds) {
    // one model, or per-step constants shared by all chains (desc.step_model: the transition into step t and the observation at t use the
    // constants of model step_model[t]) — with or without `missing` values; per-chain models keep the sequential schedule
    const bool stepm = ds->step_model != nullptr && ds->n_models > 1;
    const bool chainm = !stepm && ds->chain_model != nullptr && ds->n_models > 1;   // one model per chain (with `missing` values: else the fully observed MFMA path has them)
    if (!(ds->allow_missing || stepm) || (ds->chain_model && !chainm) || (!stepm && !chainm && ds->n_models != 1) || e->T < 2 ||
        e->hooks.gseq || ((stepm || chainm) && e->hooks.stepm_gseq))
        return RXHIP_OK;
    // the masked kernels work on d×d tiles that also hold the observation-space matrices: pad to the larger of d and dy
    e->m_dpad = 16 * ((std::max(e->d, e->dy) + 15) / 16);
    e->m_nt = e->m_dpad / 16;
    const size_t NM = (stepm || chainm) ? (size_t)ds->n_models : 1;
    e->m_chainm = chainm;
    e->m_models = (int)NM;
    e->m_stepm = stepm;
    const size_t D = (size_t)e->m_dpad, MM = D * D, C = (size_t)e->n_chains, T = (size_t)e->T;
    // Segments and the kind of boundary recursion: a cost model over the sequential depths, in µs per step from the measured kernels
    // (profiles/r03/dense_missing_parallel_kernels.txt; d = 64: fused element step 32, sweep step forward + backward 27, a round of fused
    // compositions 44, a sequential boundary step 21, a sequential group combine 50; d ≤ 16: 10 / 5.7 / 12 / 8 / 15) and the workgroups
    // the chip holds at once.  One chain at T = 2000: S = 250 segments of 8 steps, 8 rounds of compositions (log depth); chains that fill
    // the machine on their own: ONE segment per chain — the sweep kernels run the whole chain, no element pass and no boundary recursion.
    long long S = 1;
    // RXHIP_MSEG_SCAN = sequential | log: the boundary recursion as one / two sequential levels, or in ⌈log₂ S⌉ rounds (default: the cheaper one)
    const int scan_mode = e->hooks.mseg_one_level ? 1 : e->hooks.mseg_scan;
    auto hs_fits = [&](long long s) { return (double)C * (double)s * (MSEG_WS + 9 + 12) * MM * 8.0 <= 6e9; };   // scratch + elements + four generations
    auto hs_rounds_of = [](long long s) { int r = 0; while ((1LL << r) <= s - 2) ++r; return r; };
    const double f = (double)(e->m_nt - 1) / 3.0, c_s = 8.0 + f * 13.0, c_g = 15.0 + f * 35.0;
    // workgroups in flight: km_elements, km_compose and km_apply carry a register bound of their own (blocks inlined, one operand staged
    // through LDS: ≤ 256 registers) — 8, 4, 2, 2 workgroups per CU at d = 16 / 32 / 48 / 64, like the sweep kernels; the non-inlined
    // blocks of km_group / km_scan take 280 – 312 registers at d ≥ 48 (one workgroup per CU; their grids are small)
    const double conc = e->m_nt == 1 ? 2048.0 : e->m_nt == 2 ? 1024.0 : 512.0;
    const double conc_c = conc, c_c = 8.0 + f * 22.0;    // a round of fused compositions: 30 µs at d = 64 with a CU to itself, 44 µs when workgroups share one
    // log-depth recursion over ⌈s / g⌉ entries of g segments: km_fold (g − 1 compositions in a row), the rounds, km_apply, km_inner (g − 1 steps)
    const int grp_forced = e->hooks.mseg_group;
    auto log_cost = [&](long long s, int g) {
        const double n = std::ceil((double)s / (double)g), wv = std::ceil(2.0 * (double)C * n / conc_c), wf = std::ceil((double)C * n / conc_c);
        const double sh2 = 2.0 * (double)C * n > 0.5 * conc_c ? 1.45 : 1.0, sh1 = (double)C * n > 0.5 * conc_c ? 1.45 : 1.0;   // workgroups that share a CU
        return (double)(g - 1) * (c_c * wf * sh1 + 1.8 * c_s * wv * sh2) + ((double)hs_rounds_of((long long)n) * c_c + 1.8 * c_s) * wv * sh2;
    };
    auto log_group = [&](long long s) {   // the group size with the cheapest recursion
        if (grp_forced > 0) return (int)std::min<long long>(grp_forced, s);
        int gb = 1;
        for (int g = 2; g <= 8 && 2 * g <= s; g *= 2)
            if (log_cost(s, g) < log_cost(s, gb)) gb = g;
        return gb;
    };
    {
        const double c_e = 10.0 + f * 22.0, c_f = 5.7 + f * 21.0;   // fused element step (32 µs at d = 64 with every CU busy), forward + backward sweep step
        const bool w8_ok = e->m_nt == 1 && e->d <= 8 && !stepm && !chainm && !e->hooks.wave8_off;
        auto cost = [&](long long s_asked) {
            // (the segments that s_asked turns into once the segment length is an integer: ⌈(T − 1) / L⌉ of length L = ⌈(T − 1) / s_asked⌉)
            const long long Lq = ((long long)T - 1 + s_asked - 1) / s_asked, s = ((long long)T - 1 + Lq - 1) / Lq;
            const double steps = (double)Lq, rounds = std::ceil((double)C * (double)s / conc);
            double scan = 0.0;
            if (s >= 16) {
                const double sg = std::ceil(std::sqrt((double)s)), ng = std::ceil((double)s / sg);
                scan = (sg * c_g + (ng + 2.0 * sg) * c_s) * std::ceil((double)C * ng / conc);
            } else if (s > 1)
                scan = (double)s * c_s * std::ceil(2.0 * (double)C / conc);
            if (s > 2 && scan_mode != 1 && hs_fits(s)) {   // log-depth: ⌈log₂⌉ rounds of compositions, one parallel boundary step
                const double lg = log_cost(s, log_group(s));
                if (lg < scan || scan_mode == 2) scan = lg;
            }
            const double share = e->m_nt >= 3 && (double)C * (double)s > 0.5 * conc ? 1.3 : 1.0;   // d ≥ 48: two workgroups on a CU step 1.3× slower than one (narrower ones: measured neutral)
            // one segment per chain at d ≤ 8 runs inside one wavefront per chain (dense8_kernels.hpp): 1.1 + 0.75 µs per step measured with
            // one wavefront per SIMD (1024 chains), ≈ 1.4 µs per step and 1024 chains beyond that
            if (s == 1 && w8_ok) return (double)C <= 1024.0 ? steps * 1.85 : ((double)C / 1024.0) * steps * 1.4;
            return rounds * steps * share * ((s > 1 ? c_e : 0.0) + c_f) + scan;
        };
        double best = 0.7 * cost(1);   // (the interpolated element costs are optimistic between d = 16 and 64: leave one segment only for a clear win)
        for (long long s = 2; s <= (long long)T - 1; s = std::max(s + 1, (long long)((double)s * 1.15))) {
            if ((double)C * (double)s * (MSEG_WS + 9) * MM * 8.0 > 6e9) break;   // scratch of the element pass: chains × S blocks
            const double c = cost(s);
            if (c < best) { best = c; S = s; }
        }
    }
    if (ds->segments > 0) S = ds->segments;
    if (S > (long long)T - 1) S = (long long)T - 1;
    if (S < 1) S = 1;
    long long L = ((long long)T - 1 + S - 1) / S;
    S = ((long long)T - 1 + L - 1) / L;
    e->mS = (int)S; e->mL = L;
    // two-level boundary recursion from 16 segments on: groups of ≈√S segments (km_group, km_scan levels 2 / 3)
    e->m_sg = 0; e->m_ng = 0;
    e->m_hs = 0; e->m_hs_rounds = 0;
    {   // the boundary recursion of this S: sequential (one level, or two from 16 segments on) or log-depth, by the same cost figures
        double seq = (double)S * c_s * std::ceil(2.0 * (double)C / conc);
        if (S >= 16 && !e->hooks.mseg_one_level) {
            const double sg = std::ceil(std::sqrt((double)S)), ng = std::ceil((double)S / sg);
            seq = (sg * c_g + (ng + 2.0 * sg) * c_s) * std::ceil((double)C * ng / conc);
        }
        const int g = S > 2 ? log_group(S) : 1;
        const double lg = log_cost(S, g);
        e->m_hs_g = 1; e->m_hs_n = (int)S;
        if (S > 2 && hs_fits(S) && scan_mode != 1 && (lg < seq || scan_mode == 2)) {
            e->m_hs = 1;
            e->m_hs_g = g;
            e->m_hs_n = (int)((S + g - 1) / g);
            e->m_hs_rounds = hs_rounds_of(e->m_hs_n);
        }
    }
    if (!e->m_hs && S >= 16 && !e->hooks.mseg_one_level) {
        int sg = 1;
        while ((long long)sg * sg < S) ++sg;
        e->m_sg = sg;
        e->m_ng = (int)((S + sg - 1) / sg);
    }
    const size_t NG = (size_t)(e->m_hs && e->m_hs_g > 1 ? e->m_hs_n : e->m_ng > 0 ? e->m_ng : 1);   // group elements (km_group, or km_fold)
    const size_t HS = e->m_hs ? (size_t)C * (size_t)e->m_hs_n * 4 : 1;   // entries of the two generations of both scans
    const DenseCst cl = DenseCst::make((int)D, e->dy);
    const int rec = dense_rec(e->m_nt), tri = dense_tri(e->m_nt);
    const size_t nws = std::max<size_t>((size_t)C * (size_t)S, (size_t)2 * C) * MSEG_WS * MM;
    static_assert(TabWs::T6 == 15, "kt_consts works in the first 16 workspace slots");
    const size_t CWN = 16 * MM;   // kt_consts touches the named slots up to TabWs::T6 only: 16 matrices per model (the table builder's workspace has 83)
    const size_t parts[] = {NM * (5 * MM + D), NM * CWN, NM * (size_t)cl.size, C * T, C, C * S * 3 * MM, C * S * 2 * D, C * S * 2 * MM, C * S * MM, nws,
                            C * T * (size_t)rec, C * S * (size_t)tri, C * S * D, C * (S + 1) * D,
                            (2 * (size_t)S + 2 + NM * (size_t)fe_resid_blocks(e->T, e->m_dpad, e->dy)) * C, C * NG * 3 * MM, C * NG * 2 * D, C,
                            NM * ((sizeof(DenseModel) + 7) / 8), HS * 3 * MM, HS * 2 * D};
    size_t off[22] = {0};
    for (int q = 0; q < 21; ++q) off[q + 1] = off[q] + ArenaPlan::al(sizeof(double) * parts[q]);
    // The block holds per-step records for every chain (C·T·rec doubles: 4.5 KB per chain-step at d ≤ 16, 67 KB at d = 64) on top of what the
    // sequential schedule needs (the posteriors): d = 8 × 1024 chains × T = 10⁵ would ask for 460 GB.  An engine whose block does not fit
    // stays on the sequential schedule (k_gseq_*: one workgroup per chain) instead of failing — the only schedule these engines had before
    // round 3.  RXHIP_MSEG_MAX_BYTES caps the block (tests).
    {
        size_t free_b = 0, total_b = 0;
        bool fits = hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)off[21] <= 0.9 * (double)free_b;
        fits = fits && off[21] <= e->hooks.mseg_max_bytes;
        if (!fits || hipMalloc(&e->mseg_block, off[21]) != hipSuccess) {
            (void)hipGetLastError();
            e->mseg_block = nullptr;
            return RXHIP_OK;   // e->mseg stays false
        }
    }
    auto mseg_give_up = [&]() {   // a preparation step failed: release the block, keep the sequential schedule
        (void)hipGetLastError();
        (void)hipStreamSynchronize(e->stream);
        (void)hipFree(e->mseg_block);
        e->mseg_block = nullptr;
        e->d_filt = e->d_vend = e->d_fstart_m = e->d_beta_xi = nullptr;
        return RXHIP_OK;
    };
    auto at = [&](int q) { return (double*)(e->mseg_block + off[q]); };
    e->m_in = at(0); e->m_cw = at(1); e->m_cst = at(2); e->m_obs = at(3); e->m_nobs = at(4); e->m_el = at(5); e->m_vec = at(6); e->m_bnd = at(7);
    e->m_lb = at(8); e->m_ws = at(9); e->d_filt = at(10); e->d_vend = at(11); e->d_fstart_m = at(12); e->d_beta_xi = at(13); e->m_fe_part = at(14);
    e->m_grp = at(15); e->m_gvec = at(16); e->m_feconst = at(17); e->m_modtab = reinterpret_cast<DenseModel*>(at(18));
    e->m_hsel = at(19); e->m_hsvec = at(20);
    // the models padded to d×d (copies only) and their constant blocks, built on the device (one kt_consts launch per model)
    const size_t IN1 = 5 * MM + D, CW1 = CWN;
    const size_t nmod = (sizeof(DenseModel) * NM + 7) / 8;
    PinnedTmp pin(sizeof(double) * (NM * IN1 + nmod));   // padded models | model table: uploads from pinned memory (see PinnedTmp)
    if (!pin.p) return mseg_give_up();
    double* hin = pin.p;
    std::memset(hin, 0, sizeof(double) * NM * IN1);
    const int du = ds->d, dyu = ds->dy;
    for (size_t m = 0; m < NM; ++m) {
        double* h = hin + m * IN1;
        const double *Am = ds->A + m * (size_t)du * du, *Pm = ds->P + m * (size_t)du * du, *Vm = ds->V0 + m * (size_t)du * du;
        const double *Bm = ds->B + m * (size_t)dyu * du, *Qm = ds->Q + m * (size_t)dyu * dyu, *m0m = ds->m0 + m * (size_t)du;
        for (int i = 0; i < (int)D; ++i)
            for (int j = 0; j < (int)D; ++j) {
                const bool in = i < du && j < du;
                h[(size_t)i * D + j] = in ? Am[(size_t)i * du + j] : 0.0;
                h[MM + (size_t)i * D + j] = in ? Pm[(size_t)i * du + j] : (i == j ? 1.0 : 0.0);
                h[2 * MM + (size_t)i * D + j] = in ? Vm[(size_t)i * du + j] : (i == j ? 1.0 : 0.0);
                h[3 * MM + (size_t)i * D + j] = (i < dyu && j < du) ? Bm[(size_t)i * du + j] : 0.0;
                h[4 * MM + (size_t)i * D + j] = (i < dyu && j < dyu) ? Qm[(size_t)i * dyu + j] : (i == j && i >= dyu ? 1.0 : 0.0);
            }
        for (int i = 0; i < du; ++i) h[5 * MM + i] = m0m[i];
    }
    HIPCHK(e, hipMemcpyAsync(e->m_in, hin, sizeof(double) * NM * IN1, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemsetAsync(e->m_cst, 0, sizeof(double) * NM * (size_t)cl.size, e->stream));
    HIPCHK(e, hipMemsetAsync(e->m_fe_part, 0, sizeof(double) * parts[14], e->stream));
    HIPCHK(e, hipMemsetAsync(e->d_filt, 0, sizeof(double) * parts[10], e->stream));
    hipError_t herr = hipSuccess;
    const size_t lds_c = sizeof(double) * (size_t)(blk_scratch_doubles(e->m_nt) + 2 * 64 * e->m_nt + 16 + D * (D + 1));
    { const int nt_prep = e->m_nt; herr = once_per_device_checked(120 + nt_prep, e->device, [nt_prep] { return dense_vt(nt_prep)->mseg_prepare(); }); }
    if (!herr) {   // one workgroup per model
        TabParams tp{};
        tp.d = (int)D; tp.dy = e->dy; tp.ptt = e->ptt; tp.T = e->T; tp.L = 1; tp.Llast = 1; tp.S = 0; tp.sg = 1; tp.ng = 1;
        tp.in = e->m_in; tp.ws = e->m_cw; tp.cst = e->m_cst; tp.status = e->d_status;
        tp.in_stride = (long long)IN1; tp.ws_stride = (long long)CW1; tp.cst_stride = cl.size;
        dense_vt(e->m_nt)->tab_consts(tp, (unsigned)NM, lds_c, e->stream);
    }
    DenseModel* hmod = reinterpret_cast<DenseModel*>(pin.p + NM * IN1);
    for (size_t m = 0; m < NM; ++m) hmod[m] = DenseModel{e->m_cst + m * (size_t)cl.size, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!herr) herr = hipMemcpyAsync(e->m_modtab, hmod, sizeof(DenseModel) * NM, hipMemcpyHostToDevice, e->stream);
    if (herr != hipSuccess || hipGetLastError() != hipSuccess) return mseg_give_up();   // e.g. a part without 160 KB of LDS per workgroup
    HIPCHK(e, hipStreamSynchronize(e->stream));   // the pinned block goes back to the pool here
    e->mseg = true;
    return RXHIP_OK;
}
static rxhip_status mseg_run(rxhip_engine* e, bool fe, bool filter) {
    MsegParams mp{};
    mp.d = e->m_dpad; mp.dy = e->dy; mp.dy_user = e->dy; mp.ptt = e->ptt; mp.T = e->T; mp.L = e->mL; mp.n_chains = e->n_chains; mp.S = e->mS;
    mp.y = e->d_y; mp.in = e->m_in; mp.cw = e->m_cw; mp.ws = e->m_ws; mp.obs = e->m_obs; mp.nobs = e->m_nobs; mp.mel = e->m_el; mp.mvec = e->m_vec;
    mp.mbnd = e->m_bnd; mp.mlb = e->m_lb; mp.fstart_m = e->d_fstart_m; mp.beta_xi = e->d_beta_xi; mp.filt = e->d_filt; mp.rec = dense_rec(e->m_nt);
    mp.status = e->d_status;
    mp.sg = e->m_sg; mp.ng = e->m_ng; mp.mgrp = e->m_grp; mp.mgvec = e->m_gvec;
    mp.hs = e->m_hs; mp.hs_rounds = e->m_hs_rounds; mp.hsel = e->m_hsel; mp.hsvec = e->m_hsvec; mp.hs_n = e->m_hs_n; mp.hs_g = e->m_hs_g;
    const DenseCst clm = DenseCst::make(e->m_dpad, e->dy);
    mp.step_model = e->m_stepm ? e->d_step_model : nullptr;
    mp.chain_model = e->m_chainm ? e->d_chain_model : nullptr;
    mp.in_stride = 5LL * e->m_dpad * e->m_dpad + e->m_dpad; mp.cw_stride = 16LL * e->m_dpad * e->m_dpad; mp.cst_stride = clm.size;
    mp.cst = e->m_cst; mp.fe_const = e->m_feconst; mp.oC0 = (int)clm.oC0; mp.oLDP = (int)clm.oLDP;
    DenseParams dp{};
    dp.T = e->T; dp.n_chains = e->n_chains; dp.S = e->mS; dp.L = e->mL; dp.d = e->m_dpad; dp.d_out = e->d; dp.dy = e->dy; dp.pack = 1; dp.d_sub = 8; dp.dy_sub = e->dy;
    dp.y = e->d_y; dp.filt = e->d_filt; dp.vend = e->d_vend; dp.mean = e->d_mean; dp.cov = e->d_cov; dp.cst = e->m_cst;
    dp.fstart_m = e->d_fstart_m; dp.beta_xi = e->d_beta_xi; dp.fe_part = e->m_fe_part; dp.status = e->d_status;
    dp.mseg = 2;   // 2: the boundary vector of a segment is the information vector ξ_f(b_s), not the mean
    dp.obs = e->m_obs; dp.nobs = e->m_nobs; dp.mbnd = e->m_bnd;
    dp.step_model = mp.step_model; dp.cst_stride = clm.size; dp.fe_const = e->m_feconst; dp.model_sel = 0; dp.oW_off = clm.oW;
    if (e->m_chainm) { dp.models = e->m_modtab; dp.chain_model = e->d_chain_model; }   // the sweep kernels' own per-chain lookup (dense_model)
    // chains that run as ONE segment (they fill the chip on their own) at d ≤ 8: the sweep inside one wavefront per chain
    // (dense8_kernels.hpp; smoothing runs of one model; RXHIP_WAVE8=0: the MFMA kernels, which stay the checker)
    dp.wave8 = (e->mS == 1 && e->m_nt == 1 && e->d <= 8 && !e->m_stepm && !e->m_chainm && !filter && !e->hooks.wave8_off) ? 1 : 0;
    e->m_wave8_last = dp.wave8 != 0;
    if (dp.wave8) mp.rec = K8_REC;   // km_gy writes B′Q⁻¹y_t into the records the in-wave kernels read
    rxhip_status st;
    if ((st = prof_begin(e, RXHIP_K_SEG_AGGREGATE))) return st;
    dense_vt(e->m_nt)->mseg_sweep(mp, dp, fe, filter, e->stream);
    if ((st = prof_end(e))) return st;
    if (fe) launch_fe_resid(dp, e->stream, e->m_stepm ? e->m_models : 1);
    if (filter) {   // q(x_t | y_1..t) from the forward records — after the residual forms have read the smoothed means
        dense_vt(e->m_nt)->mseg_filter_out(mp, dp, e->stream);
    }
    return RXHIP_OK;
}


// Per-model tables of the dense path: constants, per-offset gains (K_i, U_i), and the data-independent
// matrix part of the boundary scan for every segment (see dense_kernels.hpp DenseParams::scanm).
static rxhip_status build_dense_tables(rxhip_engine* e, const rxhip_lgssm_desc* ds, std::vector<double>& cst,
                                       std::vector<double>& tab, std::vector<double>& scanm, std::vector<double>& qtab,
                                       std::vector<int>& canon) {
    // ds: the model at KERNEL level (a packed pair is one block-diagonal model of dimension 16, see rxhip_lgssm_create)
    const int d = e->dpad, dy = ds->dy, du = ds->d;
    const size_t MM = (size_t)d * d;
    // padded copies of the model (identity blocks on the padding dimensions)
    std::vector<double> Ap(MM, 0.0), Pp(MM, 0.0), V0p(MM, 0.0), Bp((size_t)dy * d, 0.0), m0p(d, 0.0);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            const bool in = i < du && j < du;
            Ap[(size_t)i * d + j] = in ? ds->A[(size_t)i * du + j] : 0.0;
            Pp[(size_t)i * d + j] = in ? ds->P[(size_t)i * du + j] : (i == j ? 1.0 : 0.0);
            V0p[(size_t)i * d + j] = in ? ds->V0[(size_t)i * du + j] : (i == j ? 1.0 : 0.0);
        }
    for (int i = 0; i < dy; ++i)
        for (int j = 0; j < du; ++j) Bp[(size_t)i * d + j] = ds->B[(size_t)i * du + j];
    for (int i = 0; i < du; ++i) m0p[i] = ds->m0[i];
    const double *A = Ap.data(), *B = Bp.data(), *P = Pp.data(), *Q = ds->Q, *m0 = m0p.data(), *V0 = V0p.data();
    const DenseCst c = DenseCst::make(d, dy);
    cst.assign((size_t)c.size, 0.0);
    std::vector<double> Qi(dy * dy), G(d * dy), Lobs(MM), HF(dy * d), V1(MM), V1i(MM), m1(d), t1(MM + dy * d + d * dy),
        t2(MM + dy * d + d * dy), Lf(MM), Vf1(MM);
    double ldQ = 0, ldV1 = 0, ldLf = 0;
    if (!host::chol_inv(dy, Q, Qi.data(), &ldQ)) return fail(e, RXHIP_ERR_NOT_POSDEF, "observation noise Q is not positive definite");
    if (!host::chol_inv(d, P, t1.data(), nullptr)) return fail(e, RXHIP_ERR_NOT_POSDEF, "state noise P is not positive definite");
    host::mTm(dy, d, dy, B, Qi.data(), G.data());
    host::mm(d, dy, d, G.data(), B, Lobs.data());
    host::mm(dy, d, d, B, A, HF.data());
    if (e->ptt) {
        for (int i = 0; i < d; ++i) {
            double s = 0;
            for (int k = 0; k < d; ++k) s += A[i * d + k] * m0[k];
            m1[i] = s;
        }
        host::mm(d, d, d, A, V0, t1.data());
        host::mmT(d, d, d, t1.data(), A, V1.data());
        for (size_t i = 0; i < MM; ++i) V1[i] += P[i];
    } else {
        for (int i = 0; i < d; ++i) m1[i] = m0[i];
        for (size_t i = 0; i < MM; ++i) V1[i] = V0[i];
    }
    if (!host::chol_inv(d, V1.data(), V1i.data(), &ldV1)) return fail(e, RXHIP_ERR_NOT_POSDEF, "prior covariance is not positive definite");
    for (size_t i = 0; i < MM; ++i) Lf[i] = V1i[i] + Lobs[i];
    if (!host::chol_inv(d, Lf.data(), Vf1.data(), &ldLf)) return fail(e, RXHIP_ERR_NOT_POSDEF, "first filtered precision not positive definite");
    for (size_t i = 0; i < MM; ++i) { cst[c.oA + i] = A[i]; cst[c.oP + i] = 0.5 * (P[i] + P[(i % d) * d + i / d]); cst[c.oLOBS + i] = Lobs[i]; cst[c.oVF1 + i] = Vf1[i]; }
    for (int i = 0; i < d * dy; ++i) cst[c.oG + i] = G[i];
    for (int i = 0; i < dy * dy; ++i) cst[c.oQI + i] = Qi[i];
    for (int i = 0; i < dy * d; ++i) cst[c.oHF + i] = HF[i];
    cst[c.oC0] = dy * 1.8378770664093454835606594728112 + ldQ;
    double s1 = 0;
    for (int i = 0; i < d; ++i) {
        double s = 0;
        for (int k = 0; k < d; ++k) s += V1i[i * d + k] * m1[k];
        cst[c.oX1 + i] = s;
        s1 += s * m1[i];
    }
    cst[c.oS1] = s1;
    cst[c.oLD1] = ldLf + ldV1;
    for (int i = 0; i < d; ++i) {
        double s = 0;
        for (int k = 0; k < d; ++k) s += Vf1[i * d + k] * cst[c.oX1 + k];
        cst[c.oC1 + i] = s;
    }
    host::mm(d, d, dy, Vf1.data(), G.data(), &cst[c.oK1]);
    {   // constants of the information-form smoother
        std::vector<double> Pinv(MM), Kc(MM), Wc(MM);
        double ldP = 0;
        if (!host::chol_inv(d, P, Pinv.data(), &ldP)) return fail(e, RXHIP_ERR_NOT_POSDEF, "state noise P is not positive definite");
        host::mm(d, d, d, Pinv.data(), A, Kc.data());   // K = P⁻¹A
        host::mTm(d, d, d, A, Kc.data(), Wc.data());    // W = A'(P⁻¹A)
        for (int i = 0; i < d; ++i)
            for (int k = 0; k < d; ++k) {
                cst[c.oPI + (size_t)i * d + k] = 0.5 * (Pinv[(size_t)i * d + k] + Pinv[(size_t)k * d + i]);
                cst[c.oK + (size_t)i * d + k] = Kc[(size_t)i * d + k];
                cst[c.oKT + (size_t)k * d + i] = Kc[(size_t)i * d + k];
                cst[c.oW + (size_t)i * d + k] = 0.5 * (Wc[(size_t)i * d + k] + Wc[(size_t)k * d + i]);
                cst[c.oV1I + (size_t)i * d + k] = V1i[(size_t)i * d + k];
                cst[c.oPLW + (size_t)i * d + k] = 0.5 * (Pinv[(size_t)i * d + k] + Pinv[(size_t)k * d + i]) +
                                                  0.5 * (Lobs[(size_t)i * d + k] + Lobs[(size_t)k * d + i]) +
                                                  0.5 * (Wc[(size_t)i * d + k] + Wc[(size_t)k * d + i]);
                cst[c.oPLWM + (size_t)i * d + k] = 0.5 * (Pinv[(size_t)i * d + k] + Pinv[(size_t)k * d + i]) +
                                                   0.5 * (Wc[(size_t)i * d + k] + Wc[(size_t)k * d + i]);
            }
        for (int i = 0; i < d; ++i) cst[c.oM1 + i] = m1[i];
        for (int r = 0; r < dy; ++r)
            for (int k = 0; k < d; ++k) cst[c.oBT + (size_t)k * dy + r] = B[(size_t)r * d + k];
        cst[c.oFEC] = 0.5 * (ldV1 + (double)(e->T - 1) * ldP + (double)e->T * (dy * 1.8378770664093454835606594728112 + ldQ));
        cst[c.oLDP] = ldP;
        cst[c.oLDP + 1] = ldV1;
        // whitening maps of the residual forms (kd_fe_resid_mfma): [L_P⁻¹ | −L_P⁻¹A], [L_Q⁻¹ | −L_Q⁻¹B] (zero-padded)
        std::vector<double> LPi(MM), LPiA(MM), LQi((size_t)dy * dy), LQiB((size_t)dy * d);
        if (!host::chol_linv(d, P, LPi.data())) return fail(e, RXHIP_ERR_NOT_POSDEF, "state noise P is not positive definite");
        if (!host::chol_linv(dy, Q, LQi.data())) return fail(e, RXHIP_ERR_NOT_POSDEF, "observation noise Q is not positive definite");
        host::mm(d, d, d, LPi.data(), A, LPiA.data());
        host::mm(dy, dy, d, LQi.data(), B, LQiB.data());
        const int dy4 = (dy + 3) & ~3, ky = dy4 + d;
        for (int i = 0; i < d; ++i)
            for (int k = 0; k < d; ++k) {
                cst[c.oLPX + (size_t)i * 2 * d + k] = LPi[(size_t)i * d + k];
                cst[c.oLPX + (size_t)i * 2 * d + d + k] = -LPiA[(size_t)i * d + k];
            }
        for (int i = 0; i < dy; ++i) {
            for (int k = 0; k < dy; ++k) cst[c.oLQX + (size_t)i * ky + k] = LQi[(size_t)i * dy + k];
            for (int k = 0; k < d; ++k) cst[c.oLQX + (size_t)i * ky + dy4 + k] = -LQiB[(size_t)i * d + k];
        }
    }
    for (int i = 0; i < d; ++i) {
        for (int k = 0; k < d; ++k) cst[c.oAT + (size_t)k * d + i] = A[i * d + k];
        for (int k = 0; k < dy; ++k) {
            cst[c.oGT + (size_t)k * d + i] = G[i * dy + k];
            cst[c.oK1T + (size_t)k * d + i] = cst[c.oK1 + (size_t)i * dy + k];
            cst[c.oHFT + (size_t)i * dy + k] = HF[k * d + i];
        }
    }

    // gains and element matrices (Kalman filter from an exactly known state)
    const long long L = e->L;
    // per-offset gains and closed-loop maps, kept for the aggregation tables built after the loop
    std::vector<double> Kall((size_t)L * d * dy), Uall((size_t)L * d * dy), Phiall((size_t)L * MM);
    std::vector<double> V(MM, 0.0), Pi(MM, 0.0), J(MM, 0.0), Vp(MM), S(dy * dy), Si(dy * dy), K(d * dy), HFPi(dy * d),
        U(d * dy), Phi(MM);
    struct Agg { std::vector<double> Pi, C, J, Ci, X, JJ; };
    Agg ag[2];
    for (int i = 0; i < d; ++i) Pi[i * d + i] = 1.0;
    for (long long i = 1; i <= L; ++i) {
        host::mm(d, d, d, A, V.data(), t1.data());
        host::mmT(d, d, d, t1.data(), A, Vp.data());
        for (size_t q = 0; q < MM; ++q) Vp[q] += P[q];
        host::mm(dy, d, d, B, Vp.data(), t1.data());
        host::mmT(dy, d, dy, t1.data(), B, S.data());
        for (int q = 0; q < dy * dy; ++q) S[q] += Q[q];
        if (!host::chol_inv(dy, S.data(), Si.data(), nullptr)) return fail(e, RXHIP_ERR_NOT_POSDEF, "innovation covariance not positive definite");
        host::mTm(dy, d, dy, t1.data(), Si.data(), K.data());
        host::mm(dy, d, d, HF.data(), Pi.data(), HFPi.data());
        host::mTm(dy, d, dy, HFPi.data(), Si.data(), U.data());
        host::mm(d, dy, d, U.data(), HFPi.data(), t2.data());
        for (size_t q = 0; q < MM; ++q) J[q] += t2[q];
        host::mm(d, dy, d, K.data(), t1.data(), t2.data());
        for (int a = 0; a < d; ++a)
            for (int b = 0; b <= a; ++b) {
                double s = 0.5 * ((Vp[a * d + b] - t2[a * d + b]) + (Vp[b * d + a] - t2[b * d + a]));
                V[a * d + b] = V[b * d + a] = s;
            }
        host::mm(d, dy, d, K.data(), HF.data(), t2.data());
        for (size_t q = 0; q < MM; ++q) Phi[q] = A[q] - t2[q];
        host::mm(d, d, d, Phi.data(), Pi.data(), t2.data());
        for (size_t q = 0; q < MM; ++q) Pi[q] = t2[q];
        std::copy(K.begin(), K.end(), Kall.begin() + (size_t)(i - 1) * d * dy);
        std::copy(U.begin(), U.end(), Uall.begin() + (size_t)(i - 1) * d * dy);
        std::copy(Phi.begin(), Phi.end(), Phiall.begin() + (size_t)(i - 1) * MM);
        for (int which = 0; which < 2; ++which) {
            if (i != (which == 0 ? L : e->Llast)) continue;
            Agg& g = ag[which];
            g.Pi = Pi; g.C = V; g.J = J;
            for (int a = 0; a < d; ++a) for (int b = 0; b < a; ++b) { double s = 0.5 * (g.J[a * d + b] + g.J[b * d + a]); g.J[a * d + b] = g.J[b * d + a] = s; }
            g.Ci.resize(MM); g.X.resize(MM); g.JJ.resize(MM);
            if (!host::chol_inv(d, V.data(), g.Ci.data(), nullptr)) return fail(e, RXHIP_ERR_NOT_POSDEF, "segment covariance not positive definite");
            host::mm(d, d, d, g.Ci.data(), Pi.data(), g.X.data());
            host::mTm(d, d, d, Pi.data(), g.X.data(), g.JJ.data());
            for (size_t q = 0; q < MM; ++q) g.JJ[q] += g.J[q];
        }
    }
    // Aggregation tables (kd_agg_gemm).  A segment's element (b_s, η_s) — the filtered mean from a zero start and the
    // accumulated information vector — is LINEAR in the segment's observations: with Φ_i = A − K_i (BA),
    //   b_s = Σ_i Ψ_i y_i,  Ψ_i = Φ_L ⋯ Φ_{i+1} K_i ;     η_s = Σ_i Θ_i y_i,  Θ_i = U_i − Z_i K_i,  Z_{i−1} = U_i (BA) + Z_i Φ_i, Z_L = 0
    // so the sequential per-step recursion becomes one [2d × L·dy]·[L·dy × S] product.  Two sets: full segments (length L) and the
    // last one (length Llast).  Layout [set][k = (i−1)·dyp + j][row]: rows 0..d−1 = Ψ_i[:, j], d..2d−1 = Θ_i[:, j]; dyp = dy padded to 4.
    {
        const int dyp = (dy + 3) & ~3;
        tab.assign((size_t)2 * L * dyp * 2 * d, 0.0);
        std::vector<double> Pc(MM), Pn(MM), Z(MM), Zn(MM), Psi(d * dy), ZK(d * dy), UH(MM);
        for (int which = 0; which < 2; ++which) {
            const long long Lx = which == 0 ? L : e->Llast;
            std::fill(Pc.begin(), Pc.end(), 0.0);
            for (int a = 0; a < d; ++a) Pc[(size_t)a * d + a] = 1.0;
            std::fill(Z.begin(), Z.end(), 0.0);
            for (long long i = Lx; i >= 1; --i) {
                const double* Ki = Kall.data() + (size_t)(i - 1) * d * dy;
                const double* Ui = Uall.data() + (size_t)(i - 1) * d * dy;
                const double* Phii = Phiall.data() + (size_t)(i - 1) * MM;
                host::mm(d, d, dy, Pc.data(), Ki, Psi.data());
                host::mm(d, d, dy, Z.data(), Ki, ZK.data());
                double* te = tab.data() + ((size_t)which * L + (size_t)(i - 1)) * dyp * 2 * d;
                for (int j = 0; j < dy; ++j)
                    for (int a = 0; a < d; ++a) {
                        te[(size_t)j * 2 * d + a] = Psi[(size_t)a * dy + j];
                        te[(size_t)j * 2 * d + d + a] = Ui[(size_t)a * dy + j] - ZK[(size_t)a * dy + j];
                    }
                host::mm(d, d, d, Pc.data(), Phii, Pn.data());
                Pc = Pn;
                host::mm(d, dy, d, Ui, HF.data(), UH.data());
                host::mm(d, d, d, Z.data(), Phii, Zn.data());
                for (size_t q = 0; q < MM; ++q) Z[q] = UH[q] + Zn[q];
            }
        }
    }
    dense_schedule_ints(e);
    // boundary-scan matrices
    const int S_ = e->S;
    scanm.assign((size_t)(S_ > 0 ? S_ : 1) * 6 * MM, 0.0);
    // canonical indices (DenseParams::canon): identity until a recursion has converged, then the segment the copies come from
    canon.assign((size_t)4 * (S_ > 0 ? S_ : 1), 0);
    for (int q = 0; q < 4; ++q)
        for (int s = 0; s < S_; ++s) canon[(size_t)q * S_ + s] = s;
    if (S_ > 0) {
        // Both recursions below are Riccati iterations with constant coefficients: after a transient of a few segments the
        // boundary covariance (precision) stops changing, and with it the maps.  Once two consecutive boundaries agree entry by entry,
        // |Δ_ij| ≤ RXHIP_TAB_SAME_TOL sqrt(a_ii a_jj) (each entry on its own scale — host::spd_same), the remaining segments reuse the converged
        // maps — the tables of a d = 64, S = 250 engine otherwise cost ≈1.5 GFLOP of host arithmetic per create.
        auto same = [&](const std::vector<double>& a, const std::vector<double>& b) { return host::spd_same(d, a.data(), b.data(), RXHIP_TAB_SAME_TOL); };
        std::vector<double> Vc = Vf1, Vi(MM), W(MM), M1(MM), M2(MM), tt(MM), Vprev(MM);
        bool conv = false;
        for (int s = 0; s < S_; ++s) {
            double* sm = scanm.data() + (size_t)s * 6 * MM;
            if (conv) {  // maps 0, 1 and V(b_s) of the previous segment
                std::copy(sm - 6 * MM, sm - 3 * MM, sm);
                if (s < S_ - 1) canon[s] = canon[s - 1];   // (the last segment has no step map: its slots 0, 1 are never read)
                continue;
            }
            for (size_t q = 0; q < MM; ++q) sm[2 * MM + q] = Vc[q];
            if (s == S_ - 1) break;
            const Agg& g = ag[0];
            if (!host::chol_inv(d, Vc.data(), Vi.data(), nullptr)) return fail(e, RXHIP_ERR_NOT_POSDEF, "boundary covariance not positive definite");
            for (size_t q = 0; q < MM; ++q) tt[q] = Vi[q] + g.J[q];
            if (!host::chol_inv(d, tt.data(), W.data(), nullptr)) return fail(e, RXHIP_ERR_NOT_POSDEF, "boundary precision not positive definite");
            host::mm(d, d, d, g.Pi.data(), W.data(), M2.data());
            host::mm(d, d, d, M2.data(), Vi.data(), M1.data());
            host::mmT(d, d, d, M2.data(), g.Pi.data(), tt.data());
            for (int a = 0; a < d; ++a)
                for (int b = 0; b < d; ++b) { sm[(size_t)b * d + a] = M1[a * d + b]; sm[MM + (size_t)b * d + a] = M2[a * d + b]; }
            Vprev = Vc;
            for (int a = 0; a < d; ++a)
                for (int b = 0; b <= a; ++b) {
                    double v = 0.5 * (tt[a * d + b] + tt[b * d + a]) + g.C[a * d + b];
                    Vc[a * d + b] = Vc[b * d + a] = v;
                }
            conv = same(Vc, Vprev);
        }
        std::vector<double> Lm(MM, 0.0), N1(MM), N2(MM), Lprev(MM);
        // scanm[s][5] = Λβ(b_{s+1}); Λβ(b_S) = 0
        conv = false;
        for (int s = S_ - 1; s >= 1; --s) {
            const Agg& g = ag[s == S_ - 1 ? 1 : 0];
            double* sm = scanm.data() + (size_t)s * 6 * MM;
            if (conv) {  // maps 3, 4 and Λβ of the following segment (both full-length segments)
                std::copy(sm + 9 * MM, sm + 12 * MM, sm + 3 * MM);
                canon[(size_t)S_ + s] = canon[(size_t)S_ + s + 1];
                continue;
            }
            for (size_t q = 0; q < MM; ++q) { sm[5 * MM + q] = Lm[q]; tt[q] = g.Ci[q] + Lm[q]; }
            if (!host::chol_inv(d, tt.data(), W.data(), nullptr)) return fail(e, RXHIP_ERR_NOT_POSDEF, "backward boundary precision not positive definite");
            host::mTm(d, d, d, g.X.data(), W.data(), N1.data());   // X' W
            host::mm(d, d, d, N1.data(), Lm.data(), N2.data());    // X' W Λ
            host::mm(d, d, d, N1.data(), g.X.data(), tt.data());   // X' W X
            for (int a = 0; a < d; ++a)
                for (int b = 0; b < d; ++b) { sm[3 * MM + (size_t)b * d + a] = N1[a * d + b]; sm[4 * MM + (size_t)b * d + a] = N2[a * d + b]; }
            Lprev = Lm;
            for (int a = 0; a < d; ++a)
                for (int b = 0; b <= a; ++b) {
                    double v = g.JJ[a * d + b] - 0.5 * (tt[a * d + b] + tt[b * d + a]);
                    Lm[a * d + b] = Lm[b * d + a] = v;
                }
            conv = s < S_ - 1 && same(Lm, Lprev);  // the last segment has its own length: compare full-length steps only
        }
        for (size_t q = 0; q < MM; ++q) scanm[5 * MM + q] = Lm[q];  // segment 0: Λβ(b_1)
    }
    // two-level scan (kd_scan_local / kd_scan_fix): groups of sg ≈ √(S−1) scan steps, composed maps Q_q (transposed)
    {
        const int n = S_ - 1;
        const int sg = e->scan_sg;
        qtab.assign((size_t)2 * (S_ > 0 ? S_ : 1) * MM, 0.0);
        std::vector<double> Mp(MM), Qc(MM), Qn(MM);
        for (int dir = 0; dir < 2 && n > 0; ++dir) {
            bool grp_same = false, qc_stale = false;
            for (int st = 0; st < n; ++st) {
                const int seg = dir ? S_ - 1 - st : st;
                const double* mt = scanm.data() + ((size_t)seg * 6 + (dir ? 3 : 0)) * MM;  // stored transposed
                // converged region of the Riccati recursions: a group whose step maps equal (bit for bit — they are copies)
                // those of the previous group has the same products
                if (st % sg == 0) grp_same = st >= sg;
                if (grp_same) {
                    const int pseg = dir ? S_ - 1 - (st - sg) : st - sg;
                    const double* pt = scanm.data() + ((size_t)pseg * 6 + (dir ? 3 : 0)) * MM;
                    grp_same = std::memcmp(pt, mt, sizeof(double) * MM) == 0;
                }
                double* qt = qtab.data() + ((size_t)dir * S_ + (st + 1)) * MM;
                if (grp_same) {
                    std::copy(qt - (size_t)sg * MM, qt - (size_t)sg * MM + MM, qt);
                    canon[(size_t)(2 + dir) * S_ + (st + 1)] = canon[(size_t)(2 + dir) * S_ + (st + 1 - sg)];
                    qc_stale = true;
                    continue;
                }
                for (int a = 0; a < d; ++a)
                    for (int b = 0; b < d; ++b) Mp[(size_t)a * d + b] = mt[(size_t)b * d + a];
                if (st % sg == 0) Qn = Mp;
                else {
                    if (qc_stale)  // the product through the previous step was copied, not computed: read it back
                        for (int a = 0; a < d; ++a)
                            for (int b = 0; b < d; ++b) Qc[(size_t)a * d + b] = (qt - MM)[(size_t)b * d + a];
                    host::mm(d, d, d, Mp.data(), Qc.data(), Qn.data());
                }
                qc_stale = false;
                Qc = Qn;
                for (int a = 0; a < d; ++a)
                    for (int b = 0; b < d; ++b) qt[(size_t)b * d + a] = Qc[(size_t)a * d + b];
            }
        }
    }
    return RXHIP_OK;
}


// ------------------------------------------------------------------------------------------
extern "C" {

const char* rxhip_version(void) { return "rxhip 0.1 (gfx950, fp64)"; }

const char* rxhip_status_string(rxhip_status s) {
    switch (s) {
        case RXHIP_OK: return "ok";
        case RXHIP_ERR_BADARG: return "bad argument";
        case RXHIP_ERR_UNSUPPORTED: return "unsupported node type / graph shape";
        case RXHIP_ERR_NOT_POSDEF: return "matrix is not positive definite";
        case RXHIP_ERR_NONFINITE_FE: return "free energy is NaN or Inf";
        case RXHIP_ERR_HIP: return "HIP runtime error";
        case RXHIP_ERR_NO_DEVICE: return "no HIP device";
        case RXHIP_ERR_STATE: return "invalid call order";
        case RXHIP_ERR_RCCL: return "RCCL error";
        default: return "unknown status";
    }
}

int32_t rxhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int32_t rxhip_lgssm_supported(int32_t d, int32_t dy) { return (find_vtbl(d, dy) || dense_supported(d, dy)) ? 1 : 0; }

const char* rxhip_last_error(const rxhip_engine* e) { return e ? e->err.c_str() : "null engine"; }

static void free_all(rxhip_engine* e) {
    DevGuard dg;
    if (e->device >= 0) (void)dg.set(e->device);
    if (!e->dts.empty()) {  // shared tables: not this engine's to free; nothing may still read them
        if (e->stream) (void)hipStreamSynchronize(e->stream);
        e->d_cst = e->d_tab = e->d_scanm = e->d_qtab = e->d_bnd = nullptr;
        e->d_canon = nullptr;
        for (DenseTables* dt : e->dts) dense_tables_release(dt);
        e->dts.clear();
    }
    e->d_models = nullptr;  // lives in the arena
    if (e->mseg_block) e->d_filt = e->d_vend = e->d_fstart_m = e->d_beta_xi = nullptr;  // carved from mseg_block (freed below)
    free_buffers(e, {&e->d_vtab, &e->d_scan, &e->d_filt, &e->d_mean, &e->d_cov, &e->d_cst, &e->d_tab, &e->d_agg, &e->d_elem,
                     &e->d_fstart, &e->d_beta, &e->d_fe_part, &e->d_fe_chain, &e->d_fe_total});
    if (e->own_y && e->d_y && !e->in_arena(e->d_y)) (void)hipFree(e->d_y);
    e->d_y = nullptr;
    if (e->d_chain_model && !e->in_arena(e->d_chain_model)) (void)hipFree(e->d_chain_model);
    if (e->d_status && !e->in_arena(e->d_status)) (void)hipFree(e->d_status);
    if (e->d_fe_blocks && !e->in_arena(e->d_fe_blocks)) (void)hipFree(e->d_fe_blocks);
    if (family_of(e).release) family_of(e).release(e);   // the family's own sub-object
    free_buffers(e, {&e->d_scanm, &e->d_fstart_m, &e->d_beta_xi, &e->d_vend, &e->d_qtab, &e->d_loc, &e->d_aggpart, &e->d_bnd});
    if (e->d_coll) { (void)hipFree(e->d_coll); e->d_coll = nullptr; }
    if (e->mseg_block) { (void)hipFree(e->mseg_block); e->mseg_block = nullptr; }
    if (e->noise_block) { (void)hipFree(e->noise_block); e->noise_block = nullptr; }
    if (e->n_hist) { (void)hipFree(e->n_hist); e->n_hist = nullptr; }
    if (e->d_bq) { (void)hipFree(e->d_bq); e->d_bq = nullptr; }
    if (e->d_stream) { (void)hipFree(e->d_stream); e->d_stream = nullptr; }
    if (e->h_stream) { (void)hipHostFree(e->h_stream); e->h_stream = nullptr; }
    if (e->h_io) { pinned_release(e->h_io, e->h_io_bytes); e->h_io = nullptr; }
    if (e->d_off_chain) { (void)hipFree(e->d_off_chain); e->d_off_chain = nullptr; }
    for (auto& pe : e->pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto ev : e->pool) (void)hipEventDestroy(ev);
    if (e->ev_tab0) { (void)hipEventDestroy(e->ev_tab0); e->ev_tab0 = nullptr; }
    if (e->ev_tab1) { (void)hipEventDestroy(e->ev_tab1); e->ev_tab1 = nullptr; }
    e->pending.clear();
    e->pool.clear();
    if (e->stream) (void)hipStreamSynchronize(e->stream);  // nothing of this engine may still be running on its buffers
    if (e->h_stage) { pinned_release(e->h_stage, e->h_stage_bytes); e->h_stage = nullptr; }   // (the creation upload has long finished)
    if (e->own_stream && e->stream) stream_release(e->device, e->stream);
    e->stream = nullptr;
    if (e->arena) arena_release(e->device, e->arena, e->arena_bytes);
    e->arena = nullptr;
}

// ---- engine pool ---------------------------------------------------------------------------------------------------------------
// `infer(...)` of the reference builds its model per call, and so does the mirror: for the problems the reference's own benchmark runs
// (one chain, d ≤ 4, T = 50 … 50 000) constructing and destroying the engine — host table arithmetic, the arena, the upload, the stream —
// is 0.08 ms of a 0.2 ms call.  rxhip_destroy therefore PARKS a small engine instead of freeing it, and rxhip_lgssm_create hands a parked
// engine out again when the descriptor is the same, byte for byte (shapes, schedule options, device, every model matrix): nothing is
// recomputed, because nothing would come out different.  Poolable: the d, dy ≤ 4 family, one model, no masks / per-step constants / offsets /
// horizon / caller's stream, T · chains ≤ 2¹⁶.  An engine that ever reported an error is not parked.  At most 4 engines (oldest evicted);
// rxhip_release_cached_memory() empties the pool; RXHIP_ENGINE_POOL=0 (RXHIP_TEST_HOOKS=1) switches it off for A/B measurements.
struct EnginePool {
    std::mutex m;
    std::vector<rxhip_engine*> idle;   // most recently parked last
};
static EnginePool& engine_pool() {
    static EnginePool* p = new EnginePool;   // intentionally leaked, like the other pools
    return *p;
}
static bool engine_pool_on() {
    if (!caching_on()) return false;
    const char* v = hook_env("RXHIP_ENGINE_POOL");
    return !(v && std::atoi(v) == 0);
}
static bool engine_pool_key(const rxhip_lgssm_desc* ds, const ScheduleHooks& hooks, std::string& key) {
    key.clear();
    if (!engine_pool_on()) return false;
    if (ds->d > 4 || ds->dy > 4 || ds->n_models != 1 || ds->chain_model || ds->step_model || ds->state_offset || ds->obs_offset || ds->allow_missing ||
        ds->horizon != 0 || ds->stream || (long long)ds->T * ds->n_chains > 65536)
        return false;
    auto put = [&](const void* q, size_t n) { key.append((const char*)q, n); };
    int dev = ds->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return false;   // "the current device" is part of the key as the device it is NOW
    const long long hdr[7] = {ds->d, ds->dy, ds->T, ds->n_chains, ds->prior_through_transition ? 1 : 0, ds->segments, dev};
    put(hdr, sizeof hdr);
    const size_t d = (size_t)ds->d, dy = (size_t)ds->dy;
    put(ds->A, 8 * d * d); put(ds->B, 8 * dy * d); put(ds->P, 8 * d * d); put(ds->Q, 8 * dy * dy); put(ds->m0, 8 * d); put(ds->V0, 8 * d * d);
    hooks.append_key(key);   // every schedule hook: an engine of another schedule is another engine
    return true;
}
static void engine_pool_flush() {
    std::vector<rxhip_engine*> old;
    {
        EnginePool& ep = engine_pool();
        std::lock_guard<std::mutex> g(ep.m);
        old.swap(ep.idle);
    }
    for (rxhip_engine* e : old) { free_all(e); delete e; }
}

rxhip_status rxhip_set_caching(int32_t enabled) {
    g_caching.store(enabled ? 1 : 0, std::memory_order_relaxed);
    if (!enabled) return rxhip_release_cached_memory();   // what is idle goes now; what live handles hold goes with them
    return RXHIP_OK;
}
rxhip_status rxhip_release_cached_memory(void) {
    engine_pool_flush();
    dense_tables_trim(0, 0);
    ArenaPool& ap = arena_pool();
    std::lock_guard<std::mutex> g(ap.m);
    for (auto& b : ap.idle) {
        DevGuard dg;
        (void)dg.set(b.device);
        (void)hipFree(b.p);
    }
    ap.idle.clear();
    ap.total = 0;
    PinnedPool& pp = pinned_pool();
    std::lock_guard<std::mutex> g2(pp.m);
    for (auto& b : pp.idle) (void)hipHostFree(b.p);
    pp.idle.clear();
    return RXHIP_OK;
}

rxhip_status rxhip_destroy(rxhip_engine* e) {
    if (!e) return RXHIP_OK;
    if (e->tree) {
        if (e->d_coll) {   // scratch of rxhip_allreduce_free_energy
            DevGuard dg;
            (void)dg.set(e->device);
            (void)hipStreamSynchronize(e->stream);
            (void)hipFree(e->d_coll);
        }
        rxhip::tree::destroy(e->tree);
        delete e;
        return RXHIP_OK;
    }
    if (!e->pool_key.empty() && e->err.empty() && !e->profiling && e->pending.empty() && e->stream && engine_pool_on()) {
        DevGuard dg;
        if (e->device >= 0) (void)dg.set(e->device);
        if (hipStreamSynchronize(e->stream) == hipSuccess) {   // nothing of the previous owner is still running
            rxhip_engine* evict = nullptr;
            {
                EnginePool& ep = engine_pool();
                std::lock_guard<std::mutex> g(ep.m);
                ep.idle.push_back(e);
                if (ep.idle.size() > 4) { evict = ep.idle.front(); ep.idle.erase(ep.idle.begin()); }
            }
            if (evict) { free_all(evict); delete evict; }
            return RXHIP_OK;
        }
    }
    free_all(e);
    delete e;
    return RXHIP_OK;
}

// known inputs: μ[t] = A μ[t-1] + c[t] (μ before the first state = 0), ν[t] = B μ[t] + d[t]; the sweep runs on x − μ, y − ν
static void offsets_to_shifts(rxhip_engine* e, const double* cx, const double* cy) {
    const size_t d = (size_t)e->d, dy = (size_t)e->dy, To = (size_t)e->Tout();
    e->h_mu.assign(To * d, 0.0);
    e->h_nu.assign(To * dy, 0.0);
    e->h_cx.assign(To * d, 0.0);
    e->h_cy.assign(To * dy, 0.0);
    if (cx) std::memcpy(e->h_cx.data(), cx, sizeof(double) * To * d);
    if (cy) std::memcpy(e->h_cy.data(), cy, sizeof(double) * To * dy);
    for (size_t t = 0; t < To; ++t) {
        const size_t mdl = e->h_offsm.empty() ? 0 : (size_t)e->h_offsm[t];
        const double *A = e->h_offA.data() + mdl * d * d, *B = e->h_offB.data() + mdl * dy * d;
        double* mu = &e->h_mu[t * d];
        if (t > 0 || e->ptt) {
            for (size_t i = 0; i < d; ++i) {
                double s = e->h_cx[t * d + i];
                if (t > 0)
                    for (size_t k = 0; k < d; ++k) s += A[i * d + k] * e->h_mu[(t - 1) * d + k];
                mu[i] = s;
            }
        }
        for (size_t a = 0; a < dy; ++a) {
            double s = e->h_cy[t * dy + a];
            for (size_t k = 0; k < d; ++k) s += B[a * d + k] * mu[k];
            e->h_nu[t * dy + a] = s;
        }
    }
}

rxhip_status rxhip_lgssm_set_offsets(rxhip_engine* e, const double* state_offset, const double* obs_offset) {
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Lgssm) return RXHIP_ERR_BADARG;
    if (!e->d_mu) return fail(e, RXHIP_ERR_STATE, "set_offsets: the engine was created without offsets (pass zero arrays at creation to reserve them)");
    if (e->off_chain) return fail(e, RXHIP_ERR_STATE, "set_offsets: this engine carries per-chain inputs (rxhip_lgssm_set_chain_offsets)");
    SET_DEVICE(e);
    // the engine's copy of the observations carries the old shift: take it out, put the new one in
    if (e->have_data) hipLaunchKernelGGL(k_shift_rows, dim3(2048), dim3(256), 0, e->stream, e->d_y, (const double*)e->d_nu, e->T, e->n_chains, e->dy, 1.0, e->off_chain ? 1 : 0);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    offsets_to_shifts(e, state_offset, obs_offset);
    HIPCHK(e, hipMemcpyAsync(e->d_mu, e->h_mu.data(), sizeof(double) * e->h_mu.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->d_nu, e->h_nu.data(), sizeof(double) * e->h_nu.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->d_cx, e->h_cx.data(), sizeof(double) * e->h_cx.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->d_cy_raw, e->h_cy.data(), sizeof(double) * e->h_cy.size(), hipMemcpyHostToDevice, e->stream));
    if (e->have_data) hipLaunchKernelGGL(k_shift_rows, dim3(2048), dim3(256), 0, e->stream, e->d_y, (const double*)e->d_nu, e->T, e->n_chains, e->dy, -1.0, e->off_chain ? 1 : 0);
    HIPCHK(e, hipGetLastError());
    return rxhip_sync(e);  // the host vectors are the copy sources
}

// Leaves cov_current (engine.hpp) alone, like the known inputs of creation: offsets shift the means (μ, ν: k_shift_rows on y and on the posterior means),
// the covariance table of the model does not see them.
rxhip_status rxhip_lgssm_set_chain_offsets(rxhip_engine* e, const double* state_offset, const double* obs_offset, int32_t layout) {
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Lgssm) return RXHIP_ERR_BADARG;
    if (layout != RXHIP_LAYOUT_TIME_CHAIN && layout != RXHIP_LAYOUT_CHAIN_TIME) return fail(e, RXHIP_ERR_BADARG, "set_chain_offsets: unknown layout %d", layout);
    if (!e->d_mu) return fail(e, RXHIP_ERR_STATE, "set_chain_offsets: the engine was created without offsets (pass zero arrays at creation to reserve them)");
    SET_DEVICE(e);
    const size_t C = (size_t)e->n_chains, To = (size_t)e->Tout(), d = (size_t)e->d, dy = (size_t)e->dy;
    const size_t n_mu = To * C * d, n_nu = To * C * dy, n_ab = e->h_offA.size() + e->h_offB.size();
    // take the old shift out of the engine's copy of the observations (shared or per chain, whatever it was)
    if (e->have_data) hipLaunchKernelGGL(k_shift_rows, dim3(2048), dim3(256), 0, e->stream, e->d_y, (const double*)e->d_nu, e->T, e->n_chains, e->dy, 1.0, e->off_chain ? 1 : 0);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (!e->d_off_chain) HIPCHK(e, hipMalloc(&e->d_off_chain, sizeof(double) * (2 * n_mu + 2 * n_nu + n_ab)));
    double *mu = e->d_off_chain, *nu = mu + n_mu, *cx = nu + n_nu, *cy = cx + n_mu, *ab = cy + n_nu;
    {   // A | B per model, interleaved per model as the kernel reads them
        std::vector<double> hab;
        const size_t M = e->h_offA.size() / (d * d);
        for (size_t m = 0; m < M; ++m) {
            hab.insert(hab.end(), e->h_offA.begin() + m * d * d, e->h_offA.begin() + (m + 1) * d * d);
            hab.insert(hab.end(), e->h_offB.begin() + m * dy * d, e->h_offB.begin() + (m + 1) * dy * d);
        }
        HIPCHK(e, hipMemcpy(ab, hab.data(), sizeof(double) * hab.size(), hipMemcpyHostToDevice));
    }
    // host [To][C][k] or [C][To][k] -> device [To][C][k].  NULL keeps what the engine was created with: the constant offsets
    // (graph constants c[t] / d[t]) replicated over the chains — NOT zeros: a model with data inputs on the transitions and a
    // constant observation offset must keep the latter
    auto put = [&](double* dst, const double* src, size_t k, const std::vector<double>& created) -> rxhip_status {
        const size_t n = To * C * k;
        std::vector<double> rep;
        int lay = layout;
        if (!src) {
            if (created.size() != To * k) { HIPCHK(e, hipMemsetAsync(dst, 0, sizeof(double) * n, e->stream)); return RXHIP_OK; }
            rep.resize(n);
            for (size_t t = 0; t < To; ++t)
                for (size_t ch = 0; ch < C; ++ch) std::memcpy(&rep[(t * C + ch) * k], &created[t * k], sizeof(double) * k);
            src = rep.data();
            lay = RXHIP_LAYOUT_TIME_CHAIN;
        }
        if (lay == RXHIP_LAYOUT_TIME_CHAIN || C == 1) { HIPCHK(e, hipMemcpy(dst, src, sizeof(double) * n, hipMemcpyHostToDevice)); return RXHIP_OK; }
        DevTmp tmp;
        HIPCHK(e, hipMalloc(&tmp.p, sizeof(double) * n));
        HIPCHK(e, hipMemcpy(tmp.p, src, sizeof(double) * n, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_transpose_rows, dim3(2048), dim3(256), 0, e->stream, (const double*)tmp.p, dst, (long long)C, (long long)To, (int)k);
        HIPCHK(e, hipStreamSynchronize(e->stream));
        return RXHIP_OK;
    };
    if (rxhip_status st = put(cx, state_offset, d, e->h_cx_const)) return st;
    if (rxhip_status st = put(cy, obs_offset, dy, e->h_cy_const)) return st;
    MuParams mp{};
    mp.To = (long long)To; mp.n_chains = e->n_chains; mp.d = e->d; mp.dy = e->dy; mp.ptt = e->ptt; mp.cx = cx; mp.cy = cy; mp.ab = ab;
    mp.step_model = e->d_step_model; mp.mu = mu; mp.nu = nu;
    hipLaunchKernelGGL(k_mu_recursion, dim3(nblk(e->n_chains, 64)), dim3(64), 0, e->stream, mp);
    HIPCHK(e, hipGetLastError());
    e->d_mu = mu; e->d_nu = nu; e->d_cx = cx; e->d_cy_raw = cy;  // the shared arrays stay where they are (arena); these take over
    e->off_chain = true;
    if (e->have_data) hipLaunchKernelGGL(k_shift_rows, dim3(2048), dim3(256), 0, e->stream, e->d_y, (const double*)e->d_nu, e->T, e->n_chains, e->dy, -1.0, 1);
    HIPCHK(e, hipGetLastError());
    // a host that forms c = B_u·u itself (the route rxhip.h describes for this entry point) has supplied the inputs of a du > 0 engine
    if (state_offset && e->du > 0) e->have_inputs = true;
    return rxhip_sync(e);
}

static std::atomic<int>& conditioning_guard() {
    static std::atomic<int> on{1};
    return on;
}
rxhip_status rxhip_set_conditioning_guard(int32_t enabled) {
    conditioning_guard().store(enabled ? 1 : 0);
    return RXHIP_OK;
}
// ---- rxhip_lgssm_create in pieces: the descriptor, the conditioning envelope, the engine pool, the engine's description and schedule
// (lgssm_plan.hpp), then one helper per kernel family (create_gseq, create_dense, create_lanes)
static rxhip_status validate_desc(const rxhip_lgssm_desc* ds, const LgssmVtbl** vt_out, bool* dense_out) {
    if (!ds || ds->d <= 0 || ds->dy <= 0 || ds->T <= 0 || ds->n_chains <= 0 || ds->n_models <= 0 || !ds->A ||
        !ds->B || !ds->P || !ds->Q || !ds->m0 || !ds->V0)
        return RXHIP_ERR_BADARG;
    const LgssmVtbl* vt = find_vtbl(ds->d, ds->dy);
    const bool dense = !vt && dense_supported(ds->d, ds->dy);
    if (dense && ds->n_models > 1 && !ds->chain_model && !ds->step_model) return RXHIP_ERR_BADARG;
    if (!vt && !dense) return RXHIP_ERR_UNSUPPORTED;
    if (ds->chain_model)
        for (long long c = 0; c < ds->n_chains; ++c)
            if (ds->chain_model[c] < 0 || ds->chain_model[c] >= ds->n_models) return RXHIP_ERR_BADARG;
    if (ds->step_model) {
        if (ds->chain_model || ds->horizon < 0) return RXHIP_ERR_BADARG;
        for (long long t = 0; t < ds->T + ds->horizon; ++t)
            if (ds->step_model[t] < 0 || ds->step_model[t] >= ds->n_models) return RXHIP_ERR_BADARG;
    }
    *vt_out = vt;
    *dense_out = dense;
    return RXHIP_OK;
}
// the information-form schedules of d > 4 are validated inside an envelope of model conditioning (model_envelope.hpp)
static rxhip_status check_envelope(const rxhip_lgssm_desc* ds) {
    const size_t dd = (size_t)ds->d * ds->d, bd = (size_t)ds->dy * ds->d, qq = (size_t)ds->dy * ds->dy;
    const double limit = ds->d <= 16 ? envelope::ENVELOPE_ONE_TILE : envelope::ENVELOPE_TILES;
    for (int m = 0; m < ds->n_models; ++m) {
        // (per-step models: every model against the prior of the chain; a model that is never the first sees V0 only through this bound)
        const double k = envelope::kappa(ds->d, ds->dy, ds->A + m * dd, ds->B + m * bd, ds->P + m * dd, ds->Q + m * qq, ds->V0 + (ds->step_model ? (size_t)ds->step_model[0] * dd : m * dd),
                                         ds->prior_through_transition != 0);
        if (std::isfinite(k) && k > limit) {
            char buf[400];
            std::snprintf(buf, sizeof buf,
                          "model %d: conditioning kappa = %.3g of its filtered precisions is beyond %.0e, the envelope the information-form chain schedules of d = %d are "
                          "validated for (csrc/model_envelope.hpp); the node-array executor holds such models (rxhip_create hands the graph to it; rxhip_set_conditioning_guard(0) "
                          "switches this check off)",
                          m, k, limit, ds->d);
            rxhip_lower::last_error() = buf;
            return RXHIP_ERR_UNSUPPORTED;
        }
    }
    return RXHIP_OK;
}
// a parked engine of exactly this descriptor and these hooks: as good as new (engine pool above)
static rxhip_engine* engine_pool_take(const std::string& pkey) {
    rxhip_engine* hit = nullptr;
    {
        EnginePool& ep = engine_pool();
        std::lock_guard<std::mutex> g(ep.m);
        for (size_t i = ep.idle.size(); i-- > 0;)
            if (ep.idle[i]->pool_key == pkey) { hit = ep.idle[i]; ep.idle.erase(ep.idle.begin() + (long)i); break; }
    }
    if (hit) {
        if (!hit->own_y) hit->d_y = nullptr;   // (a caller's device pointer of the previous life)
        static_cast<rxhip_engine_life&>(*hit) = rxhip_engine_life{};   // every per-owner field at once (engine.hpp)
    }
    return hit;
}
// the engine's description: schedule fields from the planner, host copies of what later entry points need
static rxhip_status create_describe(rxhip_engine* e, const rxhip_lgssm_desc* ds, const LgssmVtbl* vt, bool dense) {
    plan::Shape sh;
    sh.d = ds->d; sh.dy = ds->dy; sh.T = ds->T; sh.n_chains = ds->n_chains; sh.n_models = ds->n_models; sh.segments = ds->segments;
    sh.dense = dense; sh.allow_missing = ds->allow_missing != 0; sh.step_model = ds->step_model != nullptr; sh.chain_model = ds->chain_model != nullptr;
    const plan::Flags fl = plan::static_flags(sh, e->hooks);
    const plan::Segmentation sg = plan::segmentation(sh, fl, e->hooks);
    e->vt = vt;
    e->dense = dense;
    e->dpad = fl.dpad;
    e->nt = fl.nt;
    e->d = ds->d;
    e->dy = ds->dy;
    e->T = ds->T;
    e->n_chains = ds->n_chains;
    e->n_models = ds->n_models;
    e->ptt = ds->prior_through_transition ? 1 : 0;
    e->uniform = fl.uniform;
    e->gseq = fl.gseq;
    e->masked = fl.masked;
    e->sequential = fl.sequential;
    e->pack = fl.pack;
    e->wg_chains = fl.wg_chains;
    e->dyk = fl.dyk;
    e->S = sg.S;
    e->L = sg.L;
    e->Llast = sg.Llast;
    if (ds->horizon < 0) return fail(e, RXHIP_ERR_BADARG, "horizon must be non-negative");
    e->H = ds->horizon;
    if (ds->state_offset || ds->obs_offset) {
        if (ds->chain_model) return fail(e, RXHIP_ERR_UNSUPPORTED, "offsets need one model per time index (no chain_model)");
        const size_t d = (size_t)ds->d, dy = (size_t)ds->dy, To = (size_t)(ds->T + ds->horizon);
        e->h_offA.assign(ds->A, ds->A + (size_t)ds->n_models * d * d);   // kept for rxhip_lgssm_set_offsets
        e->h_offB.assign(ds->B, ds->B + (size_t)ds->n_models * dy * d);
        if (ds->step_model) e->h_offsm.assign(ds->step_model, ds->step_model + To);
        offsets_to_shifts(e, ds->state_offset, ds->obs_offset);
        e->h_cx_const = e->h_cx;
        e->h_cy_const = e->h_cy;
    }
    if (dense) {  // predictions / forecasts of the MFMA path run on the user-level constants
        const size_t dd = (size_t)ds->d * ds->d, bd = (size_t)ds->dy * ds->d, qq = (size_t)ds->dy * ds->dy, sz = 2 * dd + bd + 2 * qq;
        e->h_user.assign((size_t)ds->n_models * sz, 0.0);
        for (int m = 0; m < ds->n_models; ++m) {
            double* u = &e->h_user[(size_t)m * sz];
            std::memcpy(u, ds->A + m * dd, sizeof(double) * dd);
            std::memcpy(u + dd, ds->P + m * dd, sizeof(double) * dd);
            std::memcpy(u + 2 * dd, ds->B + m * bd, sizeof(double) * bd);
            std::memcpy(u + 2 * dd + bd, ds->Q + m * qq, sizeof(double) * qq);
            if (!host::chol_inv(ds->dy, ds->Q + m * qq, u + 2 * dd + bd + qq, nullptr))
                return fail(e, RXHIP_ERR_NOT_POSDEF, "model %d: observation noise Q is not positive definite", m);
        }
    }
    if (!dense) {
        const size_t nb = (size_t)ds->dy * ds->d, nq = (size_t)ds->dy * ds->dy;
        e->h_bq.resize((size_t)ds->n_models * (nb + nq));
        for (int m = 0; m < ds->n_models; ++m) {
            std::memcpy(&e->h_bq[(size_t)m * (nb + nq)], ds->B + (size_t)m * nb, sizeof(double) * nb);
            std::memcpy(&e->h_bq[(size_t)m * (nb + nq) + nb], ds->Q + (size_t)m * nq, sizeof(double) * nq);
        }
    }
    return RXHIP_OK;
}
// dense engines: [n_models][m0 | V0] at user level (sequential schedule, rxhip_filter_step)
static std::vector<double> dense_prior(const rxhip_engine* e, const rxhip_lgssm_desc* ds) {
    std::vector<double> prior;
    const size_t Du = (size_t)e->d, np = Du + Du * Du;
    prior.resize((size_t)e->n_models * np);
    for (int m = 0; m < e->n_models; ++m) {
        std::memcpy(&prior[(size_t)m * np], ds->m0 + (size_t)m * Du, sizeof(double) * Du);
        std::memcpy(&prior[(size_t)m * np + Du], ds->V0 + (size_t)m * Du * Du, sizeof(double) * Du * Du);
    }
    return prior;
}
// d > 4 with `missing` observations or per-step constants — no tables: the user-level constants, the priors, the outputs
static rxhip_status create_gseq(rxhip_engine* e, const rxhip_lgssm_desc* ds) {
    const std::vector<double> prior = dense_prior(e, ds);
    e->S = 0; e->L = 1; e->Llast = 1;
    once_per_device(0, e->device, [] {
        (void)hipFuncSetAttribute((const void*)k_gseq_forward, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        (void)hipFuncSetAttribute((const void*)k_gseq_backward, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
    });
    const size_t CU = (size_t)e->n_chains, Du = (size_t)e->d;
    ArenaPlan ap;
    ap.upload(&e->d_user, e->h_user.data(), sizeof(double) * e->h_user.size());
    ap.upload(&e->d_prior, prior.data(), sizeof(double) * prior.size());
    if (ds->chain_model) ap.upload(&e->d_chain_model, ds->chain_model, sizeof(int) * CU);
    if (ds->step_model) ap.upload(&e->d_step_model, ds->step_model, sizeof(int) * (size_t)(e->T + e->H));
    if (!e->h_mu.empty()) {
        ap.upload(&e->d_mu, e->h_mu.data(), sizeof(double) * e->h_mu.size());
        ap.upload(&e->d_nu, e->h_nu.data(), sizeof(double) * e->h_nu.size());
        ap.upload(&e->d_cx, e->h_cx.data(), sizeof(double) * e->h_cx.size());
        ap.upload(&e->d_cy_raw, e->h_cy.data(), sizeof(double) * e->h_cy.size());
    }
    ap.zeroed(&e->d_status, sizeof(int));
    ap.zeroed(&e->d_fe_part, sizeof(double) * CU);
    e->fe_total_cap = 16;
    ap.zeroed(&e->d_fe_total, sizeof(double) * e->fe_total_cap);
    ap.plain(&e->d_fe_blocks, sizeof(double) * ((CU + 63) / 64));
    ap.plain(&e->d_fe_chain, sizeof(double) * CU);
    ap.plain(&e->d_mean, sizeof(double) * (size_t)e->Tout() * CU * Du);
    ap.plain(&e->d_cov, sizeof(double) * (size_t)e->Tout() * CU * Du * Du);
    if (rxhip_status st = arena_commit(e, ap)) return st;
    if (rxhip_status st = mseg_setup(e, ds)) return st;
    return RXHIP_OK;
}
// kernel-level model of a packed engine: blockdiag(M8, M8) with M8 the model padded to 8 decoupled dimensions
// (A = 0, P = V0 = I, m0 = 0, B = 0 there: posterior N(0, I), no contribution to the free energy)
static void pack_pair_model(const rxhip_engine* e, const rxhip_lgssm_desc* ds, std::vector<double> (&buf)[6], rxhip_lgssm_desc& dk) {
    std::vector<double>&pA = buf[0], &pB = buf[1], &pP = buf[2], &pQ = buf[3], &pm = buf[4], &pV = buf[5];
    const int du = ds->d, dyu = ds->dy, dyk = e->dyk;
    pA.assign(256, 0.0); pP.assign(256, 0.0); pV.assign(256, 0.0); pm.assign(16, 0.0);
    pB.assign((size_t)dyk * 16, 0.0); pQ.assign((size_t)dyk * dyk, 0.0);
    for (int b = 0; b < 2; ++b) {
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 8; ++j) {
                const bool in = i < du && j < du;
                const size_t o = (size_t)(8 * b + i) * 16 + 8 * b + j;
                pA[o] = in ? ds->A[(size_t)i * du + j] : 0.0;
                pP[o] = in ? ds->P[(size_t)i * du + j] : (i == j ? 1.0 : 0.0);
                pV[o] = in ? ds->V0[(size_t)i * du + j] : (i == j ? 1.0 : 0.0);
            }
        for (int i = 0; i < du; ++i) pm[8 * b + i] = ds->m0[i];
        for (int r = 0; r < dyu; ++r) {
            for (int j = 0; j < du; ++j) pB[(size_t)(dyu * b + r) * 16 + 8 * b + j] = ds->B[(size_t)r * du + j];
            for (int q = 0; q < dyu; ++q) pQ[(size_t)(dyu * b + r) * dyk + dyu * b + q] = ds->Q[(size_t)r * dyu + q];
        }
    }
    dk.d = 16; dk.dy = dyk; dk.n_chains = e->wg_chains;
    dk.A = pA.data(); dk.B = pB.data(); dk.P = pP.data(); dk.Q = pQ.data(); dk.m0 = pm.data(); dk.V0 = pV.data();
}
// the tables of one model of the MFMA path, built by the device builder (d ≥ 32) or on the host, then shared through the table cache
static rxhip_status dense_tables_build(rxhip_engine* e, const rxhip_lgssm_desc& dm, int mdl, std::vector<unsigned char>& key, StageTrace& tr, DenseTables** out) {
    const size_t Sg = (size_t)(e->S > 0 ? e->S : 1), D = (size_t)e->dpad;
    rxhip_status st = RXHIP_OK;
    DenseTables* dt = nullptr;
    dense_schedule_ints(e);
    const bool on_dev = dense_tab_on_device(e);
    std::vector<double> cst, tab, scanm, qtab;
    std::vector<int> canon;
    const DenseCst cl = DenseCst::make((int)D, e->dyk);
    const size_t MMd = D * D, dyp4 = (size_t)((e->dyk + 3) & ~3);
    size_t nb[6];
    if (on_dev) {
        nb[0] = (size_t)cl.size; nb[1] = (size_t)2 * e->L * dyp4 * 2 * D; nb[2] = Sg * 6 * MMd; nb[3] = 2 * Sg * MMd;
        nb[4] = Sg * 2 * MMd; nb[5] = (4 * Sg + 1) / 2;
    } else {
        st = build_dense_tables(e, &dm, cst, tab, scanm, qtab, canon);
        if (st) return st;
        tr.mark("dense: host tables", STAGE_TABLES_HOST);
        nb[0] = cst.size(); nb[1] = tab.size(); nb[2] = scanm.size(); nb[3] = qtab.size(); nb[4] = Sg * 2 * MMd; nb[5] = (canon.size() + 1) / 2;
    }
    dt = new DenseTables;
    dt->key.swap(key);
    dt->device = e->device;
    dt->agg_oc = e->agg_oc; dt->agg_kc = e->agg_kc; dt->scan_sg = e->scan_sg; dt->scan_ng = e->scan_ng;
    size_t off[7] = {0};
    for (int q = 0; q < 6; ++q) off[q + 1] = off[q] + ArenaPlan::al(sizeof(double) * (nb[q] ? nb[q] : 1));
    dt->bytes = off[6];
    if (hipMalloc(&dt->block, dt->bytes) != hipSuccess) { delete dt; return fail(e, RXHIP_ERR_HIP, "hipMalloc of %zu bytes (model tables) failed", off[6]); }
    tr.mark("dense: table block (hipMalloc)", STAGE_ALLOC);
    double** dst[5] = {&dt->d_cst, &dt->d_tab, &dt->d_scanm, &dt->d_qtab, &dt->d_bnd};
    hipError_t up = hipSuccess;
    for (int q = 0; q < 5; ++q) *dst[q] = (double*)(dt->block + off[q]);
    dt->d_canon = (int*)(dt->block + off[5]);
    // device build: padded inputs | workspace | two status words, ONE temporary allocation (freed when the tables are done); the
    // inputs travel through a pinned block and the status words come back into it
    DevTmp tab_ws;
    const size_t nin = 5 * MMd + D, nws = on_dev ? TabWs::doubles((int)D, e->L) : 0;
    PinnedTmp pin(sizeof(double) * (nin + 2));
    if (!pin.p) { (void)hipFree(dt->block); delete dt; return fail(e, RXHIP_ERR_HIP, "hipHostMalloc of the staging block failed"); }
    int* h_st = reinterpret_cast<int*>(pin.p + nin);   // [0]: table builders, [2]: boundary inverses
    h_st[0] = h_st[2] = 0;
    up = hipMalloc(&tab_ws.p, sizeof(double) * ((on_dev ? nin : 0) + nws + 2));
    int* d_st = up == hipSuccess ? reinterpret_cast<int*>((double*)tab_ws.p + (on_dev ? nin : 0) + nws) : nullptr;
    if (up == hipSuccess) up = hipMemsetAsync(d_st, 0, 2 * sizeof(double), e->stream);
    tr.mark("dense: temporary workspace (hipMalloc)", STAGE_ALLOC);
    if (on_dev) {
        // the model padded to d×d (copies only): A | P | V0 | B | Q | m0 — B, Q padded to d rows, Q = I on the padding diagonal
        double* hin = pin.p;
        std::memset(hin, 0, sizeof(double) * nin);
        const int du = dm.d, dyu = dm.dy;
        for (int i = 0; i < (int)D; ++i)
            for (int j = 0; j < (int)D; ++j) {
                const bool in = i < du && j < du;
                hin[(size_t)i * D + j] = in ? dm.A[(size_t)i * du + j] : 0.0;
                hin[MMd + (size_t)i * D + j] = in ? dm.P[(size_t)i * du + j] : (i == j ? 1.0 : 0.0);
                hin[2 * MMd + (size_t)i * D + j] = in ? dm.V0[(size_t)i * du + j] : (i == j ? 1.0 : 0.0);
                hin[3 * MMd + (size_t)i * D + j] = (i < dyu && j < du) ? dm.B[(size_t)i * du + j] : 0.0;
                hin[4 * MMd + (size_t)i * D + j] = (i < dyu && j < dyu) ? dm.Q[(size_t)i * dyu + j] : (i == j && i >= dyu ? 1.0 : 0.0);
            }
        for (int i = 0; i < du; ++i) hin[5 * MMd + i] = dm.m0[i];
        if (up == hipSuccess) up = hipMemcpyAsync(tab_ws.p, hin, sizeof(double) * nin, hipMemcpyHostToDevice, e->stream);
        if (up == hipSuccess) up = hipMemsetAsync(dt->d_tab, 0, sizeof(double) * nb[1], e->stream);   // the padded k rows of the aggregation maps
        if (up == hipSuccess) up = hipMemsetAsync(dt->d_cst, 0, sizeof(double) * nb[0], e->stream);
        TabParams tp{};
        tp.d = (int)D; tp.dy = e->dyk; tp.ptt = e->ptt; tp.T = e->T; tp.L = e->L; tp.Llast = e->Llast; tp.S = e->S; tp.sg = e->scan_sg; tp.ng = e->scan_ng;
        tp.in = (const double*)tab_ws.p; tp.ws = (double*)tab_ws.p + nin; tp.cst = dt->d_cst; tp.tab = dt->d_tab; tp.scanm = dt->d_scanm;
        tp.qtab = dt->d_qtab; tp.canon = dt->d_canon; tp.status = d_st;
        if (up == hipSuccess) {
            { const int nt_prep = e->nt; up = once_per_device_checked(110 + nt_prep, e->device, [nt_prep] { return dense_vt(nt_prep)->tab_prepare(); }); }
            if (up == hipSuccess) up = dense_vt(e->nt)->tab_build(tp, e->stream);
        }
        tr.mark("dense: device tables (enqueued)", STAGE_TABLES_DEVICE);
    } else {
        const std::vector<double>* src[4] = {&cst, &tab, &scanm, &qtab};
        for (int q = 0; q < 4 && up == hipSuccess; ++q)
            up = hipMemcpyAsync(*dst[q], src[q]->data(), sizeof(double) * src[q]->size(), hipMemcpyHostToDevice, e->stream);
        if (up == hipSuccess) up = hipMemcpyAsync(dt->d_canon, canon.data(), sizeof(int) * canon.size(), hipMemcpyHostToDevice, e->stream);
    }
    if (up == hipSuccess && e->S > 0) {  // data-independent inverses at the segment boundaries: once per model, on the device
        DenseParams dp{};
        dp.S = e->S; dp.d = e->dpad; dp.dy = e->dyk; dp.scanm = dt->d_scanm; dp.bnd = dt->d_bnd; dp.canon = dt->d_canon;
        dp.status = d_st + 2;
        DENSE_DISPATCH(e->nt, prepare_bnd(dp, e->stream));
        up = hipGetLastError();
    }
    // ONE wait for the builders and the boundary inverses, then both status words out of pinned memory
    if (up == hipSuccess) up = hipMemcpyAsync(h_st, d_st, 2 * sizeof(double), hipMemcpyDeviceToHost, e->stream);
    if (up == hipSuccess) up = hipStreamSynchronize(e->stream);   // (the host vectors of the host builder die at the end of this scope)
    tr.mark(on_dev ? "dense: device tables + bnd (wait)" : "dense: table upload + bnd", on_dev ? STAGE_TABLES_DEVICE : STAGE_UPLOAD);
    if (up == hipSuccess && (h_st[0] || h_st[2])) {
        (void)hipFree(dt->block);
        delete dt;
        return fail(e, RXHIP_ERR_NOT_POSDEF, h_st[0] ? "model %d: a covariance of the model or of its filter recursion is not positive definite"
                                                     : "model %d: a boundary covariance / precision is not positive definite", mdl);
    }
    if (up != hipSuccess) {
        (void)hipFree(dt->block);
        delete dt;
        return fail(e, RXHIP_ERR_HIP, "upload of the model tables failed: %s", hipGetErrorString(up));
    }
    dense_tables_insert(dt);
    *out = dt;
    return RXHIP_OK;
}
// d > 4, fully observed, one model per chain: the MFMA path
static rxhip_status create_dense(rxhip_engine* e, const rxhip_lgssm_desc* ds) {
    const std::vector<double> prior = dense_prior(e, ds);
    StageTrace tr(e->stage_ms);
    hipError_t herr = hipSuccess;
    { const int nt_prep = e->nt; herr = once_per_device_checked(100 + nt_prep, e->device, [nt_prep] { return dense_vt(nt_prep)->prepare(); }); }
    if (herr != hipSuccess) return fail(e, RXHIP_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    const size_t C = (size_t)e->wg_chains, CU = (size_t)e->n_chains, T = (size_t)e->T, Sg = (size_t)(e->S > 0 ? e->S : 1),
                 D = (size_t)e->dpad, Du = (size_t)e->d;
    // kernel-level model: the user's, or — packed — a block-diagonal pair
    rxhip_lgssm_desc dk = *ds;
    std::vector<double> packed[6];
    if (e->pack == 2) pack_pair_model(e, ds, packed, dk);
    // the tables of every model: shared with every other engine of the same model and schedule on this device
    rxhip_status st = RXHIP_OK;
    for (int mdl = 0; mdl < e->n_models; ++mdl) {
        rxhip_lgssm_desc dm = dk;  // model `mdl` at kernel level (a packed pair has one model by construction)
        if (e->pack == 1) {
            dm.A = ds->A + (size_t)mdl * Du * Du; dm.B = ds->B + (size_t)mdl * e->dy * Du; dm.P = ds->P + (size_t)mdl * Du * Du;
            dm.Q = ds->Q + (size_t)mdl * e->dy * e->dy; dm.m0 = ds->m0 + (size_t)mdl * Du; dm.V0 = ds->V0 + (size_t)mdl * Du * Du;
        }
        std::vector<unsigned char> key;
        {
            const long long hdr[9] = {e->d, e->dy, e->T, e->S, e->L, e->Llast, e->ptt, e->dpad, e->pack};
            auto put = [&](const void* q, size_t n) { const unsigned char* b = (const unsigned char*)q; key.insert(key.end(), b, b + n); };
            put(hdr, sizeof hdr);
            const size_t o = (size_t)mdl;  // the USER's model bytes identify the tables
            put(ds->A + o * Du * Du, sizeof(double) * Du * Du); put(ds->B + o * e->dy * Du, sizeof(double) * e->dy * Du);
            put(ds->P + o * Du * Du, sizeof(double) * Du * Du); put(ds->Q + o * e->dy * e->dy, sizeof(double) * e->dy * e->dy);
            put(ds->m0 + o * Du, sizeof(double) * Du); put(ds->V0 + o * Du * Du, sizeof(double) * Du * Du);
        }
        DenseTables* dt = dense_tables_acquire(key, e->device);
        if (!dt) {
            if ((st = dense_tables_build(e, dm, mdl, key, tr, &dt))) return st;
        } else {
            e->agg_oc = dt->agg_oc; e->agg_kc = dt->agg_kc; e->scan_sg = dt->scan_sg; e->scan_ng = dt->scan_ng;
            tr.mark("dense: tables from cache", STAGE_TABLES_HOST);
        }
        e->dts.push_back(dt);  // released in free_all, whatever happens below
    }
    {
        DenseTables* dt = e->dts[0];
        e->d_cst = dt->d_cst; e->d_tab = dt->d_tab; e->d_scanm = dt->d_scanm; e->d_qtab = dt->d_qtab; e->d_bnd = dt->d_bnd;
        e->d_canon = dt->d_canon;
    }
    std::vector<DenseModel> hmodels;
    if (e->n_models > 1)
        for (DenseTables* dt : e->dts) hmodels.push_back(DenseModel{dt->d_cst, dt->d_tab, dt->d_scanm, dt->d_qtab, dt->d_bnd, dt->d_canon});
    ArenaPlan ap;
    if (e->n_models > 1) {
        ap.upload(&e->d_models, hmodels.data(), sizeof(DenseModel) * hmodels.size());
        ap.upload(&e->d_chain_model, ds->chain_model, sizeof(int) * CU);
    }
    ap.plain(&e->d_loc, sizeof(double) * C * 2 * Sg * D);
    ap.plain(&e->d_aggpart, sizeof(double) * C * (size_t)e->agg_kc * Sg * 2 * D);
    ap.zeroed(&e->d_status, sizeof(int));
    // smoothing runs use 2S slots (forward + backward parts) + one per workgroup of kd_fe_resid
    ap.zeroed(&e->d_fe_part, sizeof(double) * (2 * Sg + 2 + (size_t)fe_resid_blocks(e->T, e->dpad, e->dyk)) * CU);
    e->fe_total_cap = 16;
    ap.zeroed(&e->d_fe_total, sizeof(double) * e->fe_total_cap);
    ap.plain(&e->d_fe_blocks, sizeof(double) * ((CU + 63) / 64));
    ap.plain(&e->d_filt, sizeof(double) * C * T * dense_rec(e->nt));
    ap.plain(&e->d_vend, sizeof(double) * C * Sg * dense_tri(e->nt));
    ap.upload(&e->d_user, e->h_user.data(), sizeof(double) * e->h_user.size());
    ap.upload(&e->d_prior, prior.data(), sizeof(double) * prior.size());
    if (!e->h_mu.empty()) {
        ap.upload(&e->d_mu, e->h_mu.data(), sizeof(double) * e->h_mu.size());
        ap.upload(&e->d_nu, e->h_nu.data(), sizeof(double) * e->h_nu.size());
        ap.upload(&e->d_cx, e->h_cx.data(), sizeof(double) * e->h_cx.size());
        ap.upload(&e->d_cy_raw, e->h_cy.data(), sizeof(double) * e->h_cy.size());
    }
    ap.plain(&e->d_mean, sizeof(double) * (size_t)e->Tout() * CU * Du);
    ap.plain(&e->d_cov, sizeof(double) * (size_t)e->Tout() * CU * Du * Du);
    ap.plain(&e->d_elem, sizeof(double) * C * Sg * 2 * D);
    ap.plain(&e->d_fstart_m, sizeof(double) * C * Sg * D);
    ap.plain(&e->d_beta_xi, sizeof(double) * C * (Sg + 1) * D);
    ap.plain(&e->d_fe_chain, sizeof(double) * CU);
    e->split = e->n_models == 1 && e->S > 0 && plan::split_wanted(e->wg_chains, e->hooks);   // the model / data split (lgssm_plan.hpp)
    if (e->split) {
        const int nt_split = e->nt;
        once_per_device(16 + nt_split, e->device, [nt_split] { (void)dense_vt(nt_split)->split_prepare(); });
        ap.plain(&e->d_dtab, sizeof(double) * T * 3 * D * D);
        ap.plain(&e->d_vlast, sizeof(double) * D * D);
        ap.plain(&e->d_vstab, sizeof(double) * T * Du * Du);
        ap.plain(&e->d_fe_const, sizeof(double) * 2 * Sg);
    }
    if ((st = arena_commit(e, ap))) return st;
    tr.mark("dense: work buffers");   // (arena_commit accounts its own stages)
    return RXHIP_OK;
}
// the per-time-index maps of the one-pass schedule: data-independent, once per engine
static rxhip_status lanes_time_tables(rxhip_engine* e, bool rev_cand, int ck_forced) {
    const LgssmVtbl* vt = e->vt;
    TimeTabParams q{};
    q.T = e->T; q.L = e->L; q.pos = e->d_pos; q.scan = e->d_scan; q.mtab = e->d_mtab; q.ntab = e->d_ntab; q.vtab = e->d_vtab;
    q.status = e->d_status;
    HIPCHK(e, hipEventCreate(&e->ev_tab0));
    HIPCHK(e, hipEventCreate(&e->ev_tab1));
    HIPCHK(e, hipEventRecord(e->ev_tab0, e->stream));
    vt->time_tables(q, e->stream);
    if (e->d_gtab) {
        SmoothTabParams sq{};
        sq.T = e->T; sq.L = e->L; sq.S = e->S; sq.vtab = e->d_vtab; sq.ntab = e->d_ntab; sq.scan = e->d_scan;
        sq.gtab = e->d_gtab; sq.segend = e->d_segend; sq.blk = e->d_sblk; sq.status = e->d_status;
        sq.rev = rev_cand ? 1 : 0; sq.amp = e->d_amp; sq.ainv = e->d_ainv; sq.ckfail = e->d_ckfail;
        vt->smooth_tables(sq, e->h_cst0.data(), e->stream);
        if (rev_cand) {   // the largest stride whose windows all pass the bound (one word: a bit per failing stride 8, 16, 32)
            int ckfail = 0;
            HIPCHK(e, hipMemcpyAsync(&ckfail, e->d_ckfail, sizeof(int), hipMemcpyDeviceToHost, e->stream));
            HIPCHK(e, hipStreamSynchronize(e->stream));
            e->ck_log2 = 0;
            if (ck_forced) {
                while ((1 << e->ck_log2) < ck_forced) ++e->ck_log2;
            } else {
                for (int k = 2; k >= 0 && !e->ck_log2; --k)
                    if (!((ckfail >> k) & 1)) e->ck_log2 = 3 + k;
            }
            if (!e->ck_log2) {   // no admissible stride: the records schedule, whose F slot holds F_t (rebuild the rows)
                sq.rev = 0;
                vt->smooth_tables(sq, e->h_cst0.data(), e->stream);
            }
        }
    }
    HIPCHK(e, hipEventRecord(e->ev_tab1, e->stream));
    // no synchronisation here: the table kernels are ordered before every sweep on the engine's stream, and a covariance
    // that is not positive definite raises the status flag the first run reports (RXHIP_ERR_NOT_POSDEF)
    HIPCHK(e, hipGetLastError());
    return RXHIP_OK;
}
// d, dy ≤ 4: a lane per (chain, segment)
static rxhip_status create_lanes(rxhip_engine* e, const rxhip_lgssm_desc* ds) {
    const LgssmVtbl* vt = e->vt;
    // per-model tables
    const size_t NP = (size_t)e->d + (size_t)e->d * (e->d + 1) / 2;
    const size_t NP2 = (NP + 1) / 2;
    const size_t Ltab = e->sequential ? 0 : (size_t)e->L;  // one segment: no gain tables, no segment aggregates
    std::vector<double> cst((size_t)e->n_models * vt->cst_size), tab((size_t)e->n_models * Ltab * vt->tab_size + 1),
        agg((size_t)e->n_models * 2 * vt->agg_size), scan;
    FusedTables ft;
    const bool want_fused = plan::want_fused(e->uniform, e->S, e->n_chains, e->T, e->hooks);
    StageTrace tr(e->stage_ms);
    for (int m = 0; m < e->n_models; ++m) {
        rxhip_status st = build_model_tables(e, m, ds, cst.data() + (size_t)m * vt->cst_size,
                                             tab.data() + (size_t)m * Ltab * vt->tab_size,
                                             agg.data() + (size_t)m * 2 * vt->agg_size, e->uniform ? &scan : nullptr,
                                             want_fused ? &ft : nullptr);
        if (st) return st;
    }
    e->fused = want_fused && !scan.empty();
    e->fe_const = ft.fe_const;
    e->h_cst0.assign(cst.begin(), cst.begin() + vt->cst_size);
    tr.mark("lanes: host tables", STAGE_TABLES_HOST);
    const size_t C = (size_t)e->n_chains, T = (size_t)e->T, Sg = (size_t)(e->S > 0 ? e->S : 1);
    ArenaPlan ap;
    ap.upload(&e->d_cst, cst.data(), sizeof(double) * cst.size());
    ap.upload(&e->d_tab, tab.data(), sizeof(double) * tab.size());
    ap.upload(&e->d_agg, agg.data(), sizeof(double) * agg.size());
    if (ds->chain_model && !e->uniform) ap.upload(&e->d_chain_model, ds->chain_model, sizeof(int) * C);
    if (ds->step_model) ap.upload(&e->d_step_model, ds->step_model, sizeof(int) * (size_t)(e->T + e->H));
    if (!e->h_mu.empty()) {
        ap.upload(&e->d_mu, e->h_mu.data(), sizeof(double) * e->h_mu.size());
        ap.upload(&e->d_nu, e->h_nu.data(), sizeof(double) * e->h_nu.size());
        ap.upload(&e->d_cx, e->h_cx.data(), sizeof(double) * e->h_cx.size());
        ap.upload(&e->d_cy_raw, e->h_cy.data(), sizeof(double) * e->h_cy.size());
    }
    if (e->uniform && !scan.empty()) ap.upload(&e->d_scan, scan.data(), sizeof(double) * scan.size());
    // (reverse-filter candidates: plan::rev_cand; the stride is chosen in lanes_time_tables, once the tables exist)
    const int ck_forced = e->hooks.mean_checkpoint;
    if (ck_forced && (ck_forced < 1 || ck_forced > 32 || (ck_forced & (ck_forced - 1))))
        return fail(e, RXHIP_ERR_BADARG, "RXHIP_MEAN_CHECKPOINT=%s: a power of two from 1 to 32", e->hooks.mean_checkpoint_text.s);
    if (e->hooks.y_ring != 0 && e->hooks.y_ring != 1)
        return fail(e, RXHIP_ERR_BADARG, "RXHIP_Y_RING: 1 (the depth-1 y ring of the reverse-filter sweep) or unset (depth %d)", Y_RING_SHIPPED);
    const int waves_forced = e->hooks.sweep_waves;
    if (waves_forced < 0)
        return fail(e, RXHIP_ERR_BADARG, "RXHIP_SWEEP_WAVES: 1, 2 or 4 (wavefronts per workgroup of the reverse-filter sweep kernels) or unset");
    if (waves_forced > 1 && !plan::sweep_waves_divide(e->n_chains, waves_forced))
        return fail(e, RXHIP_ERR_BADARG, "RXHIP_SWEEP_WAVES=%d: a workgroup of %d waves takes %d chains of one segment, which does not divide the batch of %lld",
                    waves_forced, waves_forced, 64 * waves_forced, (long long)e->n_chains);
    e->sweep_waves_fwd = plan::sweep_waves(e->n_chains, plan::SWEEP_WAVES_FORWARD, waves_forced);
    e->sweep_waves_bwd = plan::sweep_waves(e->n_chains, plan::SWEEP_WAVES_BACKWARD, waves_forced);
    const bool rev_cand = plan::rev_cand(e->fused, e->n_chains, e->d, e->dy, e->T, e->hooks);
    if (e->fused) {
        ap.upload(&e->d_ftab, ft.ftab.data(), sizeof(double) * ft.ftab.size());
        ap.upload(&e->d_pos, ft.pos.data(), sizeof(double) * ft.pos.size());
        ap.upload(&e->d_fseg, ft.fseg.data(), sizeof(double) * ft.fseg.size());
        ap.plain(&e->d_mtab, sizeof(double) * T * vt->mt_row);
        ap.plain(&e->d_ntab, sizeof(double) * T * vt->mt_row);
        if (plan::gtab_tables(e->n_chains, e->hooks)) {
            ap.plain(&e->d_gtab, sizeof(double) * T * vt->gt_row);
            ap.plain(&e->d_segend, sizeof(double) * Sg * vt->se_size);
            ap.plain(&e->d_sblk, sizeof(double) * Sg * (size_t)smooth_blocks_per_segment(e->L) * 3 * e->d * e->d);
        }
        if (rev_cand) {
            ap.plain(&e->d_amp, sizeof(double) * T);
            ap.zeroed(&e->d_ainv, sizeof(double) * e->d * e->d);
            ap.zeroed(&e->d_ckfail, sizeof(int));
        }
    }
    ap.zeroed_last(&e->d_status, sizeof(int));   // status | mean | cov | fe_chain: one span (rxhip_lgssm_infer reads it back with one copy)
    ap.zeroed(&e->d_fe_part, sizeof(double) * (Sg + 2) * C);   // one slot per segment + the t = 0 update (+ the Wishart slot of a noise engine)
    e->fe_total_cap = 16;
    ap.zeroed(&e->d_fe_total, sizeof(double) * e->fe_total_cap);
    ap.plain(&e->d_fe_blocks, sizeof(double) * ((C + 63) / 64));
    if (e->uniform) {  // mean part per chain + one covariance copy per model (see lgssm_kernels.hpp store_filt_sh)
        const size_t MP2 = ((size_t)e->d + 1) / 2;
        if (!rev_cand) ap.plain(&e->d_filt, sizeof(double) * T * MP2 * 2 * (((C + 63) / 64) * 64));   // (else sized by the stride, below)
        ap.plain(&e->d_vtab, sizeof(double) * T * ((size_t)e->d * (e->d + 1) / 2));
    } else
        ap.plain(&e->d_filt, sizeof(double) * T * NP2 * 2 * (((C + 63) / 64) * 64));
    ap.plain_first(&e->d_mean, sizeof(double) * (size_t)e->Tout() * C * e->d);
    ap.plain_first(&e->d_cov, sizeof(double) * (size_t)e->Tout() * C * e->d * e->d);
    ap.plain_first(&e->d_fe_chain, sizeof(double) * C);
    ap.plain(&e->d_elem, sizeof(double) * Sg * 2 * e->d * C);
    if (e->sequential && e->S > 1) ap.plain(&e->d_elemx, sizeof(double) * Sg * vt->ex_size * C);
    ap.plain(&e->d_fstart, sizeof(double) * Sg * NP * C);
    ap.plain(&e->d_beta, sizeof(double) * (Sg + 1) * NP * C);
    // observations of small problems live in the arena too (large ones are allocated on first set_data, or never when
    // the caller hands over a device buffer)
    if (sizeof(double) * T * C * e->dy <= ((size_t)64 << 20)) {
        ap.plain(&e->d_y, sizeof(double) * T * C * e->dy);
        e->own_y = true;
    }
    if (rxhip_status st = arena_commit(e, ap)) return st;
    tr.mark("lanes: arena", -1);   // (accounted by arena_commit itself)
    if (e->fused) {
        if (rxhip_status st = lanes_time_tables(e, rev_cand, ck_forced)) return st;
        tr.mark("lanes: device tables (enqueued)", STAGE_TABLES_DEVICE);
    }
    if (rev_cand) {   // z records: one slot per checkpoint (+ the t = 0 record of the boundary scan), or one per time index
        const size_t MP2 = ((size_t)e->d + 1) / 2;
        if (e->ck_log2) e->nck = (e->L + (1LL << e->ck_log2) - 1) >> e->ck_log2;
        const size_t slots = e->ck_log2 ? 1 + Sg * (size_t)e->nck : T;
        HIPCHK(e, hipMalloc(&e->d_filt, sizeof(double) * slots * MP2 * 2 * (((C + 63) / 64) * 64)));
    }
    return RXHIP_OK;
}

rxhip_status rxhip_lgssm_create(const rxhip_lgssm_desc* ds, rxhip_engine** out) {
    if (!out) return RXHIP_ERR_BADARG;
    *out = nullptr;
    const LgssmVtbl* vt = nullptr;
    bool dense = false;
    if (rxhip_status st = validate_desc(ds, &vt, &dense)) return st;
    if (dense && conditioning_guard().load())
        if (rxhip_status st = check_envelope(ds)) return st;
    const ScheduleHooks hooks = ScheduleHooks::read(hook_env);   // once per engine: every later decision reads e->hooks
    std::string pkey;
    if (engine_pool_key(ds, hooks, pkey))
        if (rxhip_engine* hit = engine_pool_take(pkey)) {
            *out = hit;
            return RXHIP_OK;
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RXHIP_ERR_NO_DEVICE;

    rxhip_engine* e = new rxhip_engine();
    *out = e;  // returned even on failure so that rxhip_last_error is readable; caller destroys
    e->pool_key = pkey;
    e->hooks = hooks;
    if (rxhip_status st = create_describe(e, ds, vt, dense)) return st;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    if (e->gseq) return create_gseq(e, ds);
    if (dense) return create_dense(e, ds);
    return create_lanes(e, ds);
}




// A state-space chain whose observation-noise precision is unknown (include/rxhip.h, csrc/noise_kernels.hpp): an engine of the d, dy ≤ 4
// family with ONE MODEL BLOCK PER CHAIN — every chain carries its own q(W), hence its own observation-side constants, rewritten on the device
// after every sweep — on the schedule batches with per-chain models take anyway (segment elements computed in the lane).
rxhip_status rxhip_lgssm_noise_create(const rxhip_lgssm_desc* ds, const rxhip_noise_prior* pr, rxhip_engine** out) {
    if (!out) return RXHIP_ERR_BADARG;
    *out = nullptr;
    if (!ds || !pr || !pr->S0 || !pr->init_V || ds->d <= 0 || ds->dy <= 0 || ds->n_chains <= 0 || !ds->A || !ds->B || !ds->P || !ds->m0 || !ds->V0)
        return RXHIP_ERR_BADARG;
    if (!find_vtbl(ds->d, ds->dy) || ds->n_models != 1 || ds->chain_model || ds->step_model || ds->horizon || ds->allow_missing || ds->state_offset ||
        ds->obs_offset)
        return RXHIP_ERR_UNSUPPORTED;
    const size_t C = (size_t)ds->n_chains, d = (size_t)ds->d, dy = (size_t)ds->dy;
    if (!(pr->nu0 > (double)dy - 1.0) || !(pr->init_nu > (double)dy - 1.0)) return RXHIP_ERR_BADARG;
    // Q of the first sweep's host-built blocks: E_init[W]⁻¹ (k_noise_reset rewrites the Q-dependent constants at every run start anyway)
    std::vector<double> W0(dy * dy), Q0(dy * dy), S0i(dy * dy), scratch(dy * dy);
    for (size_t q = 0; q < dy * dy; ++q) W0[q] = pr->init_nu * pr->init_V[q];
    double ldS0 = 0.0;
    if (!host::chol_inv((int)dy, W0.data(), Q0.data(), nullptr) || !host::chol_inv((int)dy, pr->S0, S0i.data(), &ldS0)) return RXHIP_ERR_NOT_POSDEF;
    auto rep = [&](const double* src, size_t n) {
        std::vector<double> v(C * n);
        for (size_t c = 0; c < C; ++c) std::memcpy(&v[c * n], src, sizeof(double) * n);
        return v;
    };
    const std::vector<double> A = rep(ds->A, d * d), B = rep(ds->B, dy * d), P = rep(ds->P, d * d), Q = rep(Q0.data(), dy * dy), m0 = rep(ds->m0, d),
                              V0 = rep(ds->V0, d * d);
    std::vector<int32_t> cm(C);
    for (size_t c = 0; c < C; ++c) cm[c] = (int32_t)c;
    rxhip_lgssm_desc dd = *ds;
    dd.n_models = (int32_t)C;
    dd.A = A.data(); dd.B = B.data(); dd.P = P.data(); dd.Q = Q.data(); dd.m0 = m0.data(); dd.V0 = V0.data(); dd.chain_model = cm.data();
    // (one chain: a second, unused model block keeps the engine off the shared-model schedule, whose per-position gain tables are built
    // once from Q on the host)
    std::vector<double> A2, B2, P2, Q2, m2, V2;
    if (C == 1) {
        auto twice = [](const std::vector<double>& v) { std::vector<double> w(v); w.insert(w.end(), v.begin(), v.end()); return w; };
        A2 = twice(A); B2 = twice(B); P2 = twice(P); Q2 = twice(Q); m2 = twice(m0); V2 = twice(V0);
        dd.n_models = 2;
        dd.A = A2.data(); dd.B = B2.data(); dd.P = P2.data(); dd.Q = Q2.data(); dd.m0 = m2.data(); dd.V0 = V2.data();
    }
    if (rxhip_status st = rxhip_lgssm_create(&dd, out)) return st;
    rxhip_engine* e = *out;
    SET_DEVICE(e);
    const size_t NPR = (size_t)e->vt->noise_prior_size, NST = C * (1 + dy * dy);
    // time slices of the residual-moment pass: enough wavefronts to fill the chip (≈ 2048), at least 8 time indices per slice
    {
        const long long waves = (long long)((C + 63) / 64);
        long long sl = (2048 + waves - 1) / waves;
        sl = std::min<long long>(sl, std::min<long long>(NOISE_MAX_SLICES, std::max<long long>(1, e->T / 8)));
        e->n_slices = (int)std::max<long long>(1, sl);
    }
    size_t off[5] = {0};
    const size_t parts[4] = {dy * d, NPR, NST, (size_t)std::max(e->n_slices, e->S) * (dy * (dy + 1) / 2) * C};   // partial moments per time slice, or per segment of the sweep
    for (int q = 0; q < 4; ++q) off[q + 1] = off[q] + ArenaPlan::al(sizeof(double) * parts[q]);
    HIPCHK(e, hipMalloc(&e->noise_block, off[4]));
    e->n_B = (double*)(e->noise_block + off[0]); e->n_prior = (double*)(e->noise_block + off[1]); e->n_state = (double*)(e->noise_block + off[2]);
    e->n_part = (double*)(e->noise_block + off[3]);
    PinnedTmp pin(sizeof(double) * (dy * d + NPR));
    if (!pin.p) return fail(e, RXHIP_ERR_HIP, "hipHostMalloc of the staging block failed");
    std::memcpy(pin.p, ds->B, sizeof(double) * dy * d);
    double* hp = pin.p + dy * d;   // ν0 | S0⁻¹ | log|S0| | ν_init | V_init   (NoisePrior<DY>)
    hp[0] = pr->nu0;
    std::memcpy(hp + 1, S0i.data(), sizeof(double) * dy * dy);
    hp[1 + dy * dy] = ldS0;
    hp[2 + dy * dy] = pr->init_nu;
    std::memcpy(hp + 3 + dy * dy, pr->init_V, sizeof(double) * dy * dy);
    HIPCHK(e, hipMemcpyAsync(e->n_B, pin.p, sizeof(double) * dy * d, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->n_prior, hp, sizeof(double) * NPR, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemsetAsync(e->n_state, 0, sizeof(double) * NST, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->noise = true;
    e->pool_key.clear();   // (built on a plain engine's tables, then something else: not for the engine pool)
    return RXHIP_OK;
}

rxhip_status rxhip_lgssm_noise_continue(rxhip_engine* e, int32_t on) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (!e->noise) return fail(e, RXHIP_ERR_BADARG, "noise_continue: not an engine with an unknown noise precision");
    e->noise_continue = on != 0;
    return RXHIP_OK;
}
rxhip_status rxhip_lgssm_noise_get(rxhip_engine* e, double* nu, double* V) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (!e->noise) return fail(e, RXHIP_ERR_BADARG, "noise_get: not an engine with an unknown noise precision");
    if (!e->ran) return fail(e, RXHIP_ERR_STATE, "noise_get: no run yet");
    SET_DEVICE(e);
    const size_t C = (size_t)e->n_chains, q = (size_t)e->dy * e->dy;
    std::vector<double> st(C * (1 + q));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(st.data(), e->n_state, sizeof(double) * st.size(), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < C; ++c) {
        if (nu) nu[c] = st[c * (1 + q)];
        if (V) std::memcpy(V + c * q, &st[c * (1 + q) + 1], sizeof(double) * q);
    }
    return RXHIP_OK;
}

rxhip_status rxhip_drift_chain_create(const rxhip_drift_chain_desc* ds, rxhip_engine** out) {
    if (!out) return RXHIP_ERR_BADARG;
    *out = nullptr;
    if (!ds || ds->T <= 0 || ds->n_chains <= 0) return RXHIP_ERR_BADARG;
    if (!(ds->v0 > 0) || !(ds->obs_var > 0)) return RXHIP_ERR_NOT_POSDEF;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RXHIP_ERR_NO_DEVICE;
    rxhip_engine* e = new rxhip_engine();
    *out = e;
    e->kind = EngineKind::Drift;
    e->T = ds->T; e->n_chains = ds->n_chains; e->d = 1; e->dy = 1; e->dpad = 1;
    e->ptt = ds->prior_through_transition ? 1 : 0;
    e->dr.m0 = ds->m0; e->dr.v0 = ds->v0; e->dr.c = ds->c; e->dr.obs_var = ds->obs_var;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    const size_t C = (size_t)e->n_chains, T = (size_t)e->T;
    ArenaPlan ap;
    ap.zeroed(&e->d_status, sizeof(int));
    e->fe_total_cap = 16;
    ap.zeroed(&e->d_fe_total, sizeof(double) * e->fe_total_cap);
    ap.plain(&e->d_mean, sizeof(double) * T * C);
    ap.plain(&e->d_cov, sizeof(double) * T * C);
    ap.plain(&e->d_fe_chain, sizeof(double) * C);
    if (sizeof(double) * T * C <= ((size_t)64 << 20)) {
        ap.plain(&e->d_y, sizeof(double) * T * C);
        e->own_y = true;
    }
    return arena_commit(e, ap);
}

static rxhip_status drift_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations)) return st;
    SET_DEVICE(e);
    if (rxhip_status st = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}})) return st;
    DriftParams p;
    p.T = e->T; p.n_chains = e->n_chains; p.y = e->d_y; p.mean = e->d_mean; p.var = e->d_cov; p.fe_chain = e->d_fe_chain;
    p.m0 = e->dr.m0; p.v0 = e->dr.v0; p.c = e->dr.c; p.obs_var = e->dr.obs_var; p.ptt = e->ptt; p.status = e->d_status;
    rxhip_status st;
    for (int it = 0; it < iterations; ++it) {  // a tree: every iteration re-pushes the data and recomputes the same fixed point
        if ((st = prof_begin(e, RXHIP_K_DRIFT_CHAIN))) return st;
        if (want_fe) hipLaunchKernelGGL((k_drift_chain<true>), dim3((unsigned)e->n_chains), dim3(256), 0, e->stream, p);
        else hipLaunchKernelGGL((k_drift_chain<false>), dim3((unsigned)e->n_chains), dim3(256), 0, e->stream, p);
        if ((st = prof_end(e))) return st;
        if (want_fe) hipLaunchKernelGGL(k_sum_fixed, dim3(1), dim3(256), 0, e->stream, (const double*)e->d_fe_chain, e->n_chains, e->d_fe_total + it);
    }
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0);
    // reference-equivalent events per chain and iteration: `+`(:out), Normal(:μ), `+`(:in1) per step + the prior's message;
    // products: forward (fwd ⊗ obs) and backward (obs ⊗ bwd) at every interior state, the marginals (2 / 1 pairwise), q(x_prior)
    const uint64_t C = (uint64_t)e->n_chains, T = (uint64_t)e->T, I = (uint64_t)iterations;
    e->rule_calls = I * C * (3 * T + 1 - (e->ptt ? 0 : 2));
    e->products = I * C * (4 * (T - 1) + (e->ptt ? 2 : 0));
    e->marginals = I * C * (T + (e->ptt ? 1 : 0));
    return RXHIP_OK;
}

static rxhip_status ingest(rxhip_engine* e, const double* src, size_t n, int32_t layout, bool src_on_device) {
    if (!e) return RXHIP_ERR_BADARG;
    const size_t need = (size_t)e->T * e->n_chains * e->dy;
    if (!src || n != need) return fail(e, RXHIP_ERR_BADARG, "set_data: expected %zu doubles, got %zu", need, n);
    if (layout != RXHIP_LAYOUT_TIME_CHAIN && layout != RXHIP_LAYOUT_CHAIN_TIME)
        return fail(e, RXHIP_ERR_BADARG, "set_data: unknown layout %d", layout);
    SET_DEVICE(e);
    if (e->n_chains == 1) layout = RXHIP_LAYOUT_TIME_CHAIN;  // one chain: the two layouts coincide
    if (src_on_device && layout == RXHIP_LAYOUT_TIME_CHAIN && !e->d_nu) {  // zero-copy (not with offsets: the engine shifts its own copy)
        if (e->own_y && e->d_y && !e->in_arena(e->d_y)) HIPCHK(e, hipFree(e->d_y));
        e->d_y = const_cast<double*>(src);
        e->own_y = false;
        e->have_data = true;
        return RXHIP_OK;
    }
    if (!e->own_y || !e->d_y) {
        e->d_y = nullptr;
        HIPCHK(e, hipMalloc(&e->d_y, sizeof(double) * need));
        e->own_y = true;
    }
    if (layout == RXHIP_LAYOUT_TIME_CHAIN) {
        // host observations up to 16 MB pass through a pinned block of the pool (one memcpy on the host, then a plain DMA): a copy from
        // pageable memory makes the runtime pin the caller's pages on the spot, 1 – 8 ms for the 5 MB of BASELINE config 3 from run to run
        PinnedTmp pin(!src_on_device && sizeof(double) * need <= ((size_t)16 << 20) ? sizeof(double) * need : 0);
        if (pin.p) std::memcpy(pin.p, src, sizeof(double) * need);
        HIPCHK(e, hipMemcpyAsync(e->d_y, pin.p ? pin.p : src, sizeof(double) * need, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
    } else {
        DevTmp tmp_guard;
        const double* dsrc = src;
        if (!src_on_device) {
            HIPCHK(e, hipMalloc(&tmp_guard.p, sizeof(double) * need));
            HIPCHK(e, hipMemcpyAsync(tmp_guard.p, src, sizeof(double) * need, hipMemcpyHostToDevice, e->stream));
            dsrc = (const double*)tmp_guard.p;
        }
        // [chain][T][dy] -> [T][chain][dy]
        hipLaunchKernelGGL(k_transpose_rows, dim3(2048), dim3(256), 0, e->stream, dsrc, e->d_y, e->n_chains, e->T,
                           e->dy);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    if (e->d_nu) {  // known inputs: the sweep sees y − B μ − d
        hipLaunchKernelGGL(k_shift_rows, dim3(2048), dim3(256), 0, e->stream, e->d_y, (const double*)e->d_nu, e->T, e->n_chains, e->dy, -1.0, e->off_chain ? 1 : 0);
        HIPCHK(e, hipGetLastError());
    }
    e->have_data = true;
    return RXHIP_OK;
}

// u[t] of every chain -> c[t] = B_u u[t] (+ the constant part of the same step) -> per-chain offsets
static rxhip_status ingest_inputs(rxhip_engine* e, const double* u, size_t n, int32_t layout) {
    if (e->kind != EngineKind::Lgssm || e->du <= 0) return fail(e, RXHIP_ERR_BADARG, "set_data: this engine has no data inputs u[t]");
    const size_t C = (size_t)e->n_chains, T = (size_t)e->T, To = (size_t)e->Tout(), d = (size_t)e->d, du = (size_t)e->du;
    if (!u || n != T * C * du) return fail(e, RXHIP_ERR_BADARG, "set_data(u): expected %zu doubles, got %zu", T * C * du, n);
    if (layout != RXHIP_LAYOUT_TIME_CHAIN && layout != RXHIP_LAYOUT_CHAIN_TIME) return fail(e, RXHIP_ERR_BADARG, "set_data: unknown layout %d", layout);
    std::vector<double> c(To * C * d, 0.0);  // [t][chain][d]
    for (size_t t = 0; t < T; ++t)
        for (size_t ch = 0; ch < C; ++ch) {
            const double* ut = u + (layout == RXHIP_LAYOUT_TIME_CHAIN ? (t * C + ch) : (ch * T + t)) * du;
            double* ct = &c[(t * C + ch) * d];
            for (size_t i = 0; i < d; ++i) {
                double s = e->h_cx.empty() ? 0.0 : e->h_cx_const[t * d + i];
                if (e->h_umask[t])
                    for (size_t k = 0; k < du; ++k) s += e->h_Bu[i * du + k] * ut[k];
                ct[i] = s;
            }
        }
    // the observation offsets of the graph (constants) stay what they were: replicate them per chain
    std::vector<double> cy;
    if (!e->h_cy_const.empty()) {
        cy.resize(To * C * (size_t)e->dy);
        for (size_t t = 0; t < To; ++t)
            for (size_t ch = 0; ch < C; ++ch) std::memcpy(&cy[(t * C + ch) * e->dy], &e->h_cy_const[t * e->dy], sizeof(double) * e->dy);
    }
    const rxhip_status st = rxhip_lgssm_set_chain_offsets(e, c.data(), cy.empty() ? nullptr : cy.data(), RXHIP_LAYOUT_TIME_CHAIN);
    if (st == RXHIP_OK) e->have_inputs = true;
    return st;
}

// Neither setter touches cov_current (engine.hpp): observations and data inputs u[t] enter the means and the free energy, never the per-model
// covariance table (d_gtab / d_vstab are functions of A, B, P, Q, m0, V0 alone) — that new data costs no covariance stores is the point of the rule.
rxhip_status rxhip_set_data(rxhip_engine* e, int32_t var_id, const double* host, size_t n, int32_t layout) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    const EngineFamily& f = family_of(e);
    if (f.set_data) return f.set_data(e, var_id, host, n);
    if (var_id == RXHIP_VAR_U) return ingest_inputs(e, host, n, layout);
    if (var_id != RXHIP_VAR_Y) return fail(e, RXHIP_ERR_BADARG, "set_data: variable %d is not a data variable", var_id);
    const rxhip_status st = ingest(e, host, n, layout, false);
    return st == RXHIP_OK && f.check_data ? f.check_data(e) : st;
}
rxhip_status rxhip_set_data_device(rxhip_engine* e, int32_t var_id, const double* dev, size_t n, int32_t layout) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    const EngineFamily& f = family_of(e);
    if (f.no_device_data) return fail(e, RXHIP_ERR_BADARG, "%s", f.no_device_data);
    if (var_id != RXHIP_VAR_Y) return fail(e, RXHIP_ERR_BADARG, "set_data: variable %d is not a data variable", var_id);
    const rxhip_status st = ingest(e, dev, n, layout, true);
    return st == RXHIP_OK && f.check_data ? f.check_data(e) : st;
}

// fold finished (kernel start, kernel end) event pairs into the per-kernel sums; with `wait` the stream has been drained and
// every pair is finished.  Called from rxhip_sync and — so that long run_async loops stay bounded — from prof_begin.
static rxhip_status prof_drain(rxhip_engine* e, bool wait) {
    size_t done = 0;
    for (auto& pe : e->pending) {
        if (!wait && hipEventQuery(pe.b) != hipSuccess) break;  // events complete in stream order
        float ms = 0.f;
        HIPCHK(e, hipEventElapsedTime(&ms, pe.a, pe.b));
        e->k_ms[pe.k] += ms;
        e->k_n[pe.k] += 1;
        e->pool.push_back(pe.a);
        e->pool.push_back(pe.b);
        ++done;
    }
    e->pending.erase(e->pending.begin(), e->pending.begin() + (long)done);
    return RXHIP_OK;
}
extern "C++" rxhip_status rxhip::prof_begin(rxhip_engine* e, int k) {
    if (!e->profiling) return RXHIP_OK;
    if (e->pending.size() >= 64) {
        rxhip_status st = prof_drain(e, false);
        if (st) return st;
    }
    rxhip_engine::Pending p;
    p.k = k;
    for (hipEvent_t* ev : {&p.a, &p.b}) {
        if (!e->pool.empty()) {
            *ev = e->pool.back();
            e->pool.pop_back();
        } else
            HIPCHK(e, hipEventCreate(ev));
    }
    HIPCHK(e, hipEventRecord(p.a, e->stream));
    e->pending.push_back(p);
    return RXHIP_OK;
}
extern "C++" rxhip_status rxhip::prof_end(rxhip_engine* e) {
    if (!e->profiling) return RXHIP_OK;
    HIPCHK(e, hipEventRecord(e->pending.back().b, e->stream));
    return RXHIP_OK;
}

static rxhip_status run_impl(rxhip_engine* e, int32_t iterations, int32_t want_fe, bool filter);
rxhip_status rxhip_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (e && e->tree) return rxhip_run(e, iterations, want_fe);
    if (!e) return RXHIP_ERR_BADARG;
    return family_of(e).run(e, iterations, want_fe);
}
rxhip_status rxhip_run_filter_async(rxhip_engine* e, int32_t want_fe) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (!family_of(e).filter_twin) return fail(e, RXHIP_ERR_BADARG, "run_filter: not a state-space engine with a streaming twin (the HGF engine is a filter already)");
    return run_impl(e, 1, want_fe, true);
}
rxhip_status rxhip_filter_reset(rxhip_engine* e) {
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Lgssm) return RXHIP_ERR_BADARG;
    e->stream_k = 0;
    return RXHIP_OK;
}
rxhip_status rxhip_filter_step(rxhip_engine* e, const double* y, double* mean, double* cov, double* free_energy) {
    TREE_GUARD(e);
    if (!e || !y) return RXHIP_ERR_BADARG;
    if (e->kind != EngineKind::Lgssm) return fail(e, RXHIP_ERR_BADARG, "filter_step: not a state-space engine");
    if (!e->dense && !e->vt) return fail(e, RXHIP_ERR_UNSUPPORTED, "filter_step: no device schedule for this shape");
    e->cov_current = false; e->cov_pending = false; e->records_hold_gains = false;   // the step-wise filter writes the posterior arrays itself
    if ((e->d_step_model || e->d_cx) && e->stream_k >= e->Tout())
        return fail(e, RXHIP_ERR_STATE, "filter_step: the per-step constants / known inputs of this engine end after %lld observations", (long long)e->Tout());
    if (e->du > 0 && !e->have_inputs)
        return fail(e, RXHIP_ERR_STATE, "filter_step: this model has data inputs u[t]: call rxhip_set_data(RXHIP_VAR_U) first");
    SET_DEVICE(e);
    const size_t C = (size_t)e->n_chains, d = (size_t)e->d, dy = (size_t)e->dy, ns = e->dense ? d * d : d * (d + 1) / 2;
    const size_t o_y = C * (d + ns), o_m = o_y + C * dy, o_c = o_m + C * d, o_f = o_c + C * d * d, total = o_f + C;
    if (!e->d_stream) {
        HIPCHK(e, hipMalloc(&e->d_stream, sizeof(double) * total));
        HIPCHK(e, hipHostMalloc((void**)&e->h_stream, sizeof(double) * (total - o_y), hipHostMallocDefault));  // pinned: y | mean | cov | fe
    }
    // one pinned staging block each way: a step is H2D + kernel + D2H + one synchronisation
    std::memcpy(e->h_stream, y, sizeof(double) * C * dy);
    HIPCHK(e, hipMemcpyAsync(e->d_stream + o_y, e->h_stream, sizeof(double) * C * dy, hipMemcpyHostToDevice, e->stream));
    StreamParams sp{};
    sp.n_chains = e->n_chains; sp.k = e->stream_k; sp.ptt = e->ptt; sp.first = e->stream_k == 0;
    sp.y = e->d_stream + o_y; sp.state = e->d_stream; sp.cst = e->d_cst; sp.chain_model = e->d_chain_model;
    sp.step_model = e->d_step_model; sp.cx = e->d_cx; sp.cy = e->d_mu ? e->d_cy_raw : nullptr; sp.off_chain = e->off_chain ? 1 : 0;
    sp.mean = e->d_stream + o_m; sp.cov = e->d_stream + o_c; sp.fe = e->d_stream + o_f; sp.status = e->d_status;
    if (e->dense) {  // any d, dy ≤ 64: one workgroup per chain on the user-level constants (gseq_kernels.hpp)
        once_per_device(2, e->device, [] { (void)hipFuncSetAttribute((const void*)k_gseq_stream_step, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024); });
        GseqStreamParams gs{};
        gs.n_chains = sp.n_chains; gs.k = sp.k; gs.d = e->d; gs.dy = e->dy; gs.ptt = sp.ptt; gs.first = sp.first; gs.y = sp.y; gs.state = sp.state;
        gs.user = e->d_user; gs.prior = e->d_prior; gs.chain_model = sp.chain_model; gs.step_model = sp.step_model; gs.cx = sp.cx; gs.cy = sp.cy;
        gs.off_chain = sp.off_chain; gs.mean = sp.mean; gs.cov = sp.cov; gs.fe = sp.fe; gs.status = sp.status;
        hipLaunchKernelGGL(k_gseq_stream_step, dim3((unsigned)e->n_chains), dim3(256), gseq_lds_bytes(e->d, e->dy), e->stream, gs);
    } else
        e->vt->stream_step(sp, e->stream);
    HIPCHK(e, hipGetLastError());
    const size_t n_out = (cov || free_energy) ? total - o_m : C * d;  // mean | cov | fe are contiguous
    if (mean || cov || free_energy)
        HIPCHK(e, hipMemcpyAsync(e->h_stream + (o_m - o_y), sp.mean, sizeof(double) * n_out, hipMemcpyDeviceToHost, e->stream));
    if (rxhip_status st = rxhip_sync(e)) return st;   // a failed step (e.g. NOT_POSDEF) does not advance the per-step constants
    e->stream_k += 1;
    if (mean) std::memcpy(mean, e->h_stream + (o_m - o_y), sizeof(double) * C * d);
    if (cov) std::memcpy(cov, e->h_stream + (o_c - o_y), sizeof(double) * C * d * d);
    if (free_energy) std::memcpy(free_energy, e->h_stream + (o_f - o_y), sizeof(double) * C);
    return RXHIP_OK;
}
rxhip_status rxhip_run_filter(rxhip_engine* e, int32_t want_fe) {
    TREE_GUARD(e);
    rxhip_status st = rxhip_run_filter_async(e, want_fe);
    if (st) return st;
    return rxhip_sync(e);
}
// What one call of run_impl runs, resolved ONCE from the engine, `filter` and `want_fe` (and the engine's hooks): the iteration loop dispatches on
// these fields and evaluates no schedule predicate of its own.
enum class RunFamily { Mseg, Gseq, DenseSplit, Dense, OnePass, SmallSweep, FourPhase, Elements };
struct RunPlan {
    RunFamily family = RunFamily::Elements;
    bool filter = false, fe = false;
    bool segments = false;        // S > 0: there is a sweep beyond the boundary scan
    bool info = false;            // MFMA path: the information-form kernels (smoothing runs with S > 0), which evaluate the free energy themselves
    bool elem_full = false, no_frozen = false;   // fixed-point exits off (rxhip_set_fixed_point_exits, RXHIP_ELEM_FULL / RXHIP_NO_FROZEN)
    bool noise_in_sweep = false;  // an unknown observation-noise precision: the backward sweep leaves the residual second moments per (segment, chain) behind
    bool tinv_records = false;    // mean-only forward records behind the fixed point of V_f (k_forward_tinv / k_backward_tinv)
    bool bnd_in_sweep = false;    // reverse-filter sweep: the boundary recursion inside the waves of k_backward_sh_rev, no scan launch
    bool scan_tab = false;        // lanes: the table-driven boundary scan (boundary_scan_tab) instead of the general one
    bool backward_sh = false;     // lanes: the table-driven backward sweep (k_backward_sh / k_backward_sh_rev) instead of the lanes' own
    bool elements_pass = false;   // Elements: several segments, their elements computed in the lane (k_seg_elements)
    int fe_slots = 0;             // partial free-energy slots per chain the reduction sums (Params::S of k_fe_few / k_fe_chain)
    double* fe_part = nullptr;    // … and where they are
};
static RunPlan resolve_run(const rxhip_engine* e, bool filter, bool fe) {
    const ScheduleHooks& h = e->hooks;
    RunPlan pl;
    pl.filter = filter;
    pl.fe = fe;
    pl.segments = e->S > 0;
    pl.info = !filter && e->S > 0;
    pl.noise_in_sweep = e->noise && !e->dense && e->S > 0 && !filter && !h.noise_moments_pass;
    pl.elem_full = e->full_recursions || h.elem_full;
    pl.no_frozen = e->full_recursions || h.no_frozen;
    // per-chain, time-invariant models on long segments: mean-only forward records behind the fixed point of V_f (k_forward_tinv / k_backward_tinv)
    // (any segment length: interior segments start ON the fixed point; an unknown-noise engine's models are time-invariant within a sweep, and its
    //  separate moment pass — the test hook — reads posteriors, not records)
    pl.tinv_records = !e->dense && !e->uniform && e->d_elemx && !e->masked && !e->d_step_model && !filter && e->n_chains % 64 == 0 && e->S > 0 && !pl.elem_full &&
                      (!e->noise || pl.noise_in_sweep);
    const bool fused = e->fused && !filter;
    // k_small_sweep (lgssm_kernels.hpp): the whole four-phase sweep of a small problem in one launch.  Per-kernel profiling keeps the separate
    // launches (there is nothing to time separately in one kernel); RXHIP_SMALL_SWEEP=0 forces them (the tests compare the two bit for bit).
    const bool small = !h.small_sweep_off && !e->dense && !fused && e->uniform && !e->sequential && !e->masked && e->d_scan && e->S > 0 &&
                       e->n_chains <= 16 && e->n_chains * (long long)e->S <= 256 && !e->profiling;   // (≤ 16 chains: the free-energy reduction of k_fe_few)
    // `missing` observations / per-step constants at d > 4 on the masked MFMA schedule (smoothing; filtering runs: the same sweep, then the
    // filtered moments from its records) unless the sequential schedule is asked for as the checker of filtering runs
    const bool mseg = e->gseq && e->mseg && !(filter && h.filter_gseq);
    pl.family = mseg ? RunFamily::Mseg : e->gseq ? RunFamily::Gseq : e->dense ? (pl.info && e->split ? RunFamily::DenseSplit : RunFamily::Dense)
                : fused ? RunFamily::OnePass : small ? RunFamily::SmallSweep : (e->S > 0 && !e->sequential) ? RunFamily::FourPhase : RunFamily::Elements;
    // Reverse-filter sweep of a shared-model batch: every wave of k_backward_sh_rev runs the boundary recursion for its own segment and chains
    // (boundary_in_sweep), so the scan is no launch of its own and k_fe_seg, which reads the segment-start means, follows the sweep.
    // RXHIP_BOUNDARY_KERNEL=1 keeps the separate launch: the comparison arm of tests/test_boundary_in_sweep_gpu.py.
    pl.bnd_in_sweep = fused && e->uniform && e->d_scan && e->d_gtab && e->ck_log2 > 0 && e->S > 0 && !e->noise && !e->masked && !h.boundary_kernel;
    pl.scan_tab = e->uniform && (e->d_scan || e->S == 0);
    pl.backward_sh = fused && e->d_gtab;
    pl.elements_pass = pl.family == RunFamily::Elements && e->d_elemx;   // masked / per-step schedules with several segments
    pl.fe_slots = e->S + (e->noise ? 1 : 0);   // + the Wishart slot
    pl.fe_part = e->d_fe_part;
    if (mseg) {   // slots of kd_forward_info / kd_backward_info / kd_fe_resid over the mseg segments
        pl.fe_part = e->m_fe_part;
        pl.fe_slots = 2 * e->mS - 1 + (int)mseg_resid_slots(e->T, e->m_dpad, e->dy, e->m_stepm, e->m_models);
    }
    // residual quadratic forms at the smoothed means (parallel over all steps), then 2S partial slots of kd_forward_info / kd_backward_info + kd_fe_resid's
    if (e->dense && !e->gseq && pl.info) pl.fe_slots = 2 * e->S - 1 + fe_resid_blocks(e->T, e->dpad, e->dyk);
    return pl;
}
static Params fill_params(const rxhip_engine* e, const RunPlan& pl) {
    Params p;
    p.T = e->T;
    p.n_chains = e->n_chains;
    p.S = e->S;
    p.L = e->L;
    p.n_models = e->n_models;
    p.y = e->d_y;
    p.filt = e->d_filt;
    p.nb64 = (e->n_chains + 63) / 64;
    p.ck_log2 = e->ck_log2;
    p.nck = e->nck;
    p.ainv = e->d_ainv;
    p.vtab = e->d_vtab;
    p.scan = e->d_scan;
    p.mean = e->d_mean;
    p.cov = e->d_cov;
    p.cst = e->d_cst;
    p.tab = e->d_tab;
    p.agg = e->d_agg;
    p.chain_model = e->d_chain_model;
    p.elem = e->d_elem;
    p.fstart = e->d_fstart;
    p.beta = e->d_beta;
    p.fe_part = e->d_fe_part;
    p.fe_chain = e->d_fe_chain;
    p.fe_total = e->d_fe_total;
    p.status = e->d_status;
    p.filter = pl.filter ? 1 : 0;
    p.masked = e->masked ? 1 : 0;
    p.step_model = e->d_step_model;
    p.elemx = e->d_elemx;
    p.noise_B = pl.noise_in_sweep ? e->n_B : nullptr;
    p.noise_part = pl.noise_in_sweep ? e->n_part : nullptr;
    p.elem_full = pl.elem_full ? 1 : 0;
    p.tinv_records = pl.tinv_records ? 1 : 0;
    const bool fused = pl.family == RunFamily::OnePass;
    p.ftab = fused ? e->d_ftab : nullptr; p.mtab = fused ? e->d_mtab : nullptr; p.ntab = fused ? e->d_ntab : nullptr;
    p.fseg = fused ? e->d_fseg : nullptr; p.fe_const = e->fe_const;
    p.fe_scale = pl.filter ? 1.0 / (double)e->T : 1.0;
    return p;
}
static DenseParams fill_dense_params(const rxhip_engine* e, const RunPlan& pl) {
    DenseParams dp{};
    if (!(e->dense && !e->gseq)) return dp;
    dp.T = e->T; dp.n_chains = e->wg_chains; dp.S = e->S; dp.L = e->L; dp.d = e->dpad; dp.d_out = e->d; dp.dy = e->dyk;
    dp.pack = e->pack; dp.d_sub = 8; dp.dy_sub = e->dy;
    dp.models = e->n_models > 1 ? e->d_models : nullptr; dp.chain_model = e->d_chain_model;
    dp.y = e->d_y; dp.filt = e->d_filt; dp.vend = e->d_vend; dp.mean = e->d_mean; dp.cov = e->d_cov; dp.cst = e->d_cst; dp.tab = e->d_tab;
    dp.bnd = e->d_bnd; dp.qtab = e->d_qtab; dp.canon = e->d_canon; dp.loc = e->d_loc; dp.sg = e->scan_sg; dp.ng = e->scan_ng;
    dp.aggpart = e->d_aggpart; dp.agg_oc = e->agg_oc; dp.agg_kc = e->agg_kc; dp.Llast = e->Llast;
    dp.scanm = e->d_scanm; dp.elem = e->d_elem; dp.fstart_m = e->d_fstart_m; dp.beta_xi = e->d_beta_xi;
    dp.fe_part = e->d_fe_part; dp.status = e->d_status;
    dp.filter = pl.filter ? 1 : 0;
    dp.no_frozen = pl.no_frozen ? 1 : 0;
    return dp;
}
// a run starts from the @initialization marginal of W (iterations re-push the data: batch.jl:391-430)
static rxhip_status fill_noise_params(rxhip_engine* e, const RunPlan& pl, int32_t iterations, NoiseParams& np) {
    if (pl.filter) return fail(e, RXHIP_ERR_BADARG, "run_filter: an engine with an unknown noise precision has no streaming twin");
    const bool noise_in_sweep = pl.noise_in_sweep;
    np.T = e->T; np.n_chains = e->n_chains; np.S = e->S; np.y = e->d_y; np.mean = e->d_mean; np.cov = e->d_cov; np.B = e->n_B;
    np.cst = e->d_cst; np.prior = e->n_prior; np.state = e->n_state; np.fe_part = e->d_fe_part; np.status = e->d_status;
    np.part = e->n_part; np.slices = noise_in_sweep ? e->S : e->n_slices; np.moments_in_sweep = noise_in_sweep ? 1 : 0;
    if (iterations > e->n_hist_cap) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (e->n_hist) HIPCHK(e, hipFree(e->n_hist));
        e->n_hist = nullptr;
        HIPCHK(e, hipMalloc(&e->n_hist, sizeof(double) * (size_t)iterations * (size_t)e->n_chains * (1 + (size_t)e->dy * e->dy)));
        e->n_hist_cap = iterations;
    }
    np.hist = e->n_hist;
    if (!(e->noise_continue && e->ran)) e->vt->noise_reset(np, e->stream);
    return RXHIP_OK;
}

static rxhip_status run_mseg(rxhip_engine* e, const RunPlan& pl) {
    if (rxhip_status st = mseg_run(e, pl.fe, pl.filter)) return st;
    e->records_hold_gains = !pl.filter && !e->m_wave8_last;   // (the in-wave d ≤ 8 sweep keeps records of its own shape)
    return RXHIP_OK;
}
static rxhip_status run_gseq(rxhip_engine* e, const RunPlan& pl) {
    rxhip_status st;
    const bool fe = pl.fe, filter = pl.filter;
    GseqParams gq{};
    gq.T = e->T; gq.n_chains = e->n_chains; gq.d = e->d; gq.dy = e->dy; gq.ptt = e->ptt; gq.fe = fe ? 1 : 0; gq.y = e->d_y;
    gq.mean = e->d_mean; gq.cov = e->d_cov; gq.user = e->d_user; gq.prior = e->d_prior; gq.chain_model = e->d_chain_model;
    gq.step_model = e->d_step_model; gq.fe_part = e->d_fe_part; gq.status = e->d_status;
    const size_t lds = gseq_lds_bytes(e->d, e->dy);
    if ((st = prof_begin(e, RXHIP_K_FORWARD))) return st;
    hipLaunchKernelGGL(k_gseq_forward, dim3((unsigned)e->n_chains), dim3(256), lds, e->stream, gq);
    if ((st = prof_end(e))) return st;
    if (!filter && e->T > 1) {
        if ((st = prof_begin(e, RXHIP_K_BACKWARD))) return st;
        hipLaunchKernelGGL(k_gseq_backward, dim3((unsigned)e->n_chains), dim3(256), lds, e->stream, gq);
        if ((st = prof_end(e))) return st;
    }
    return RXHIP_OK;
}
static rxhip_status run_dense(rxhip_engine* e, const RunPlan& pl, const DenseParams& dp, bool was_cov_current, bool write_cov) {
    rxhip_status st;
    const bool fe = pl.fe, info = pl.info;
    if (pl.segments) {
        if ((st = prof_begin(e, RXHIP_K_SEG_AGGREGATE))) return st;
        DENSE_DISPATCH(e->nt, seg_aggregate(dp, e->stream));
        if ((st = prof_end(e))) return st;
    }
    // smoothing runs with S > 0 evaluate the free energy in the forward / backward kernels (information form);
    // filtering runs and single-observation chains keep the evidence terms of the scan + covariance-form forward kernel
    if ((st = prof_begin(e, RXHIP_K_BOUNDARY_SCAN))) return st;
    DENSE_DISPATCH(e->nt, boundary_scan(dp, fe && !info, e->stream));
    if ((st = prof_end(e))) return st;
    if (pl.family == RunFamily::DenseSplit) {
        SplitParams sq{};
        sq.p = dp; sq.D = e->dpad; sq.rec = dense_rec(e->nt); sq.dtab = e->d_dtab; sq.vlast = e->d_vlast; sq.vstab = e->d_vstab;
        sq.fe_const = e->d_fe_const;
        if (!e->split_ready) {  // the model pass: the full kernels on ONE workgroup chain, their records -> tables
            DenseParams mp = dp;
            mp.vlast = e->d_vlast;
            mp.full_records = 1;   // kd_split_tables reads the matrices of every time index
            DENSE_DISPATCH(e->nt, forward_info(mp, true, e->stream, 1));
            DENSE_DISPATCH(e->nt, backward_info(mp, true, e->stream, 1));
            hipLaunchKernelGGL(kd_split_tables, dim3((unsigned)e->T), dim3(256), 0, e->stream, sq);
            hipLaunchKernelGGL(kd_split_save, dim3(256), dim3(256), 0, e->stream, sq, (long long)e->n_chains);
            e->split_ready = true;
        }
        if ((st = prof_begin(e, RXHIP_K_FORWARD))) return st;
        const long long per_wg = 4 * (64 / e->dpad);  // chains of one segment per workgroup
        const dim3 lds_grid((unsigned)((e->wg_chains + per_wg - 1) / per_wg), (unsigned)e->S);
        dense_vt(e->nt)->split_forward(sq, lds_grid, e->stream);
        if ((st = prof_end(e))) return st;
        if ((st = prof_begin(e, RXHIP_K_BACKWARD))) return st;
        dense_vt(e->nt)->split_backward(sq, lds_grid, e->stream);
        // covariances: when the array does not hold them already (mode 0: write_cov, the rule of run_impl), or (mode 1) when somebody asks
        // for them; the constant free-energy slots every sweep
        const bool lazy = e->cov_mode == 1 && e->H == 0;
        if (lazy && was_cov_current) e->cov_current = true;   // nothing in this schedule touches the array
        else if (lazy) e->cov_pending = true;
        const bool store = !lazy && write_cov;
        hipLaunchKernelGGL(kd_split_broadcast, dim3(store ? 2048 : 64), dim3(256), 0, e->stream, sq, (long long)e->n_chains, fe ? 1 : 0, store ? 1 : 0);
        if ((st = prof_end(e))) return st;
    } else if (pl.segments) {
        if ((st = prof_begin(e, RXHIP_K_FORWARD))) return st;
        if (info) { DENSE_DISPATCH(e->nt, forward_info(dp, fe, e->stream, -1)); }
        else { DENSE_DISPATCH(e->nt, forward(dp, fe, e->stream)); }
        if ((st = prof_end(e))) return st;
        if (info) {
            if ((st = prof_begin(e, RXHIP_K_BACKWARD))) return st;
            DENSE_DISPATCH(e->nt, backward_info(dp, fe, e->stream, -1));
            e->records_hold_gains = e->pack == 1;
            if ((st = prof_end(e))) return st;
        }
    }
    return RXHIP_OK;
}
static rxhip_status run_lanes(rxhip_engine* e, const RunPlan& pl, const Params& p, bool write_cov) {
    rxhip_status st;
    const bool fe = pl.fe, fused = pl.family == RunFamily::OnePass, bnd_in_sweep = pl.bnd_in_sweep;
    if (fused) {  // one pass over the observations: known-start recursion + z_t records + evidence parts
        if ((st = prof_begin(e, RXHIP_K_FORWARD))) return st;
        e->vt->forward0(p, e->h_cst0.data(), fe, e->ck_log2 > 0, e->sweep_waves_fwd, e->stream);
        if ((st = prof_end(e))) return st;
    } else if (pl.family == RunFamily::SmallSweep) {   // a few chains, a short series: aggregate, boundary scan, forward, backward and the free energy in ONE launch
        e->vt->small_sweep(p, e->h_cst0.data(), fe, e->stream);
        return RXHIP_OK;
    } else if (pl.family == RunFamily::FourPhase) {
        if ((st = prof_begin(e, RXHIP_K_SEG_AGGREGATE))) return st;
        e->vt->seg_aggregate(p, e->h_cst0.data(), e->uniform, e->stream);
        if ((st = prof_end(e))) return st;
    } else if (pl.elements_pass) {  // masked / per-step schedules with several segments: the elements are computed in the lane
        if ((st = prof_begin(e, RXHIP_K_SEG_AGGREGATE))) return st;
        e->vt->seg_elements(p, e->stream);
        if ((st = prof_end(e))) return st;
    }
    if (!bnd_in_sweep) {
        if ((st = prof_begin(e, RXHIP_K_BOUNDARY_SCAN))) return st;
        if (pl.scan_tab) e->vt->boundary_scan_tab(p, e->h_cst0.data(), fe, e->stream);
        else e->vt->boundary_scan(p, e->h_cst0.data(), e->uniform, fe, e->stream);
        if ((st = prof_end(e))) return st;
    }
    if (pl.segments) {
        if (!fused) {
            if ((st = prof_begin(e, RXHIP_K_FORWARD))) return st;
            e->vt->forward(p, e->h_cst0.data(), e->uniform, fe, e->stream);
            if ((st = prof_end(e))) return st;
        } else if (fe && !bnd_in_sweep)
            e->vt->fe_seg(p, e->stream);
        if (!pl.filter) {
            if ((st = prof_begin(e, RXHIP_K_BACKWARD))) return st;
            if (pl.backward_sh) {
                SweepArgs a;
                a.rev = e->ck_log2 > 0;
                a.bnd = bnd_in_sweep ? (fe ? 2 : 1) : 0;
                a.write_cov = write_cov;
                a.y_ring = e->hooks.y_ring == 1 ? 1 : Y_RING_SHIPPED;
                a.waves = e->sweep_waves_bwd;
                e->vt->backward_sh(p, e->h_cst0.data(), e->d_gtab, e->d_segend, a, e->stream);
            } else e->vt->backward(p, e->h_cst0.data(), e->uniform, e->stream);
            if ((st = prof_end(e))) return st;
        }
        if (fe && bnd_in_sweep) e->vt->fe_seg(p, e->stream);
    }
    return RXHIP_OK;
}
// after the sweep of every family: q(W) of a noise engine, the free-energy reduction, known inputs, the unobserved tail
static rxhip_status run_tail(rxhip_engine* e, const RunPlan& pl, const Params& p, const DenseParams& dp, NoiseParams& np, int it) {
    rxhip_status st;
    if (e->noise) {   // q(W) of every chain from this sweep's q(x); its free-energy slot; the constants of the next sweep
        np.iteration = it;
        e->vt->noise_update(np, e->stream);
    }
    if (pl.fe && pl.family != RunFamily::SmallSweep) {
        if ((st = prof_begin(e, RXHIP_K_FE_REDUCE))) return st;
        const int nb = (int)((e->n_chains + 63) / 64);
        Params pr = p;
        pr.S = pl.fe_slots;
        pr.fe_part = pl.fe_part;
        if (pl.info && (pl.family == RunFamily::Dense || pl.family == RunFamily::DenseSplit)) launch_fe_resid(dp, e->stream);
        if (e->n_chains <= 16) {
            hipLaunchKernelGGL(k_fe_few, dim3(1), dim3(256), 0, e->stream, pr);
        } else {
            hipLaunchKernelGGL(k_fe_chain, dim3(nb), dim3(256), 0, e->stream, pr, e->d_fe_blocks);
            hipLaunchKernelGGL(k_fe_total, dim3(1), dim3(256), 0, e->stream, p, (const double*)e->d_fe_blocks, nb);
        }
        if ((st = prof_end(e))) return st;
    }
    if (e->d_mu) {  // known inputs: back from x − μ to x (the free-energy terms above are invariant under the shift)
        hipLaunchKernelGGL(k_shift_rows, dim3(2048), dim3(256), 0, e->stream, e->d_mean, (const double*)e->d_mu, e->T, e->n_chains, e->d, 1.0, e->off_chain ? 1 : 0);
    }
    if (e->H > 0 && e->dense) {  // the unobserved tail on the MFMA path: generic-dimension forecast, one workgroup per chain
        GenericParams gp{};
        gp.T = e->T; gp.H = e->H; gp.n_chains = e->n_chains; gp.d = e->d; gp.dy = e->dy; gp.mean = e->d_mean; gp.cov = e->d_cov;
        gp.user = e->d_user; gp.cx = e->d_cx; gp.off_chain = e->off_chain ? 1 : 0; gp.chain_model = e->d_chain_model; gp.step_model = e->d_step_model; gp.status = e->d_status;
        hipLaunchKernelGGL(k_forecast_generic, dim3((unsigned)e->n_chains), dim3(256), generic_forecast_lds(e->d), e->stream, gp);
    }
    if (e->H > 0 && !e->dense) {  // the unobserved tail: forward messages from the last filtered (= smoothed) belief
        PredictParams pp{};
        pp.T = e->T; pp.H = e->H; pp.n_chains = e->n_chains; pp.mean = e->d_mean; pp.cov = e->d_cov; pp.cst = e->d_cst;
        pp.chain_model = e->d_chain_model; pp.step_model = e->d_step_model; pp.status = e->d_status; pp.cx = e->d_cx; pp.off_chain = e->off_chain ? 1 : 0;
        e->vt->forecast(pp, e->stream);
    }
    return RXHIP_OK;
}

// The run of a state-space engine: smoothing (the family row's run) or, with `filter`, its streaming twin (rxhip_run_filter, rxhip_lgssm_infer).
static rxhip_status run_impl(rxhip_engine* e, int32_t iterations, int32_t want_fe, bool filter) {
    if (rxhip_status st = run_preamble(e, iterations)) return st;
    const bool was_cov_current = e->cov_current && !filter;
    e->cov_current = false;   // any run may rewrite the posterior arrays; the shared-model smoothing schedules say otherwise below
    e->cov_pending = false;
    e->records_hold_gains = false;
    // the reference refuses to run while a datavar has no value (batch.jl:387-407): so does an engine whose graph has data inputs
    if (e->du > 0 && !e->have_inputs) return fail(e, RXHIP_ERR_STATE, "run: this model has data inputs u[t]: call rxhip_set_data(RXHIP_VAR_U) first");
    SET_DEVICE(e);
    if (rxhip_status st = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}})) return st;
    const bool fe = want_fe != 0;
    const RunPlan pl = resolve_run(e, filter, fe);
    Params p = fill_params(e, pl);
    const DenseParams dp = fill_dense_params(e, pl);
    NoiseParams np{};
    if (e->noise)
        if (rxhip_status st = fill_noise_params(e, pl, iterations, np)) return st;
    // Shared-model smoothing sweeps copy the covariances from a per-model table that is built at creation (d_gtab, d_vstab): no data, run or
    // iteration changes a bit of what they store.  Such a run stores the per-chain array only when it does not hold the broadcast already
    // (rxhip_engine_life::cov_current, engine.hpp: the writers of d_cov and what keeps the state true).  RXHIP_COV_EVERY_SWEEP=1 (test hook):
    // every sweep stores it, the comparison arm of tests/test_cov_once_gpu.py.  Mode 1 of the split schedule keeps its own bookkeeping (run_dense).
    const bool cov_once = !e->hooks.cov_every_sweep && !pl.filter && !e->noise && e->H == 0 &&
                          ((pl.family == RunFamily::OnePass && pl.backward_sh && pl.segments) || (pl.family == RunFamily::DenseSplit && e->cov_mode == 0));
    const bool cov_lazy = pl.family == RunFamily::DenseSplit && e->cov_mode == 1 && e->H == 0;
    for (int it = 0; it < iterations; ++it) {
        p.iteration = it;
        const bool write_cov = !cov_once || (it == 0 && !was_cov_current);
        // an unknown-noise engine writes the posteriors of a run's LAST iteration only (rxhip_get_marginals is defined as that; the moments q(W) needs
        // are formed inside the sweep): 160 B/U of stores per earlier iteration that nothing ever read
        p.skip_marginals = (pl.noise_in_sweep && it + 1 < iterations) ? 1 : 0;
        rxhip_status st;
        switch (pl.family) {
            case RunFamily::Mseg: st = run_mseg(e, pl); break;
            case RunFamily::Gseq: st = run_gseq(e, pl); break;
            case RunFamily::DenseSplit:
            case RunFamily::Dense: st = run_dense(e, pl, dp, was_cov_current, write_cov); break;
            default: st = run_lanes(e, pl, p, write_cov); break;
        }
        if (!st) st = run_tail(e, pl, p, dp, np, it);
        if (st) return st;
        if (!filter && !p.skip_marginals && !cov_lazy && write_cov) e->cov_writes += 1;   // rxhip_get_covariance_writes
    }
    HIPCHK(e, hipGetLastError());
    if (cov_once) e->cov_current = true;   // rows 0 … T−1 hold what the next smoothing sweep would store
    finish_run(e, iterations, fe, filter);
    e->records_tinv = p.tinv_records != 0 && iterations > 0;
    // reference-equivalent operation counts (6 rule calls, 4 products per step)
    const uint64_t C = (uint64_t)e->n_chains, T = (uint64_t)e->T, I = (uint64_t)iterations;
    if (filter) {
        // one-step graph per observation: prior MvN(:out), `*`_A(:out), MvN_x(:out), MvN_y(:μ), `*`_B(:in) -> 5 rule
        // calls, 1 product for q(x_t) (without the transition at t = 1 when the prior sits on x[1]: 3 rule calls)
        e->rule_calls = C * (e->ptt ? 5 * T : 5 * T - 2);
        e->products = C * T;
        e->marginals = C * T;
        return RXHIP_OK;
    }
    e->rule_calls = I * C * (e->ptt ? 6 * T + 1 : 6 * T - 3);
    e->products = I * C * (e->ptt ? 4 * T - 2 : (T == 1 ? 1 : 4 * T - 4));
    e->marginals = I * C * (e->ptt ? T + 1 : T);
    return RXHIP_OK;
}
static rxhip_status lgssm_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) { return run_impl(e, iterations, want_fe, false); }

// The family table (engine.hpp): the rows of the two families of this unit, the node-array executor's empty row, and the lookup.
extern "C++" const EngineFamily& rxhip::family_of(const rxhip_engine* e) {
    //                                 run              filter  check    set_data  no_device_data  fe_total  has_x  release
    static const EngineFamily lgssm = {lgssm_run_async, true,   nullptr, nullptr,  nullptr,        nullptr,  true,  nullptr},
                              drift = {drift_run_async, false,  nullptr, nullptr,  nullptr,        nullptr,  true,  nullptr}, tree = {};
    switch (e->kind) {
        case EngineKind::Lgssm: return lgssm;
        case EngineKind::Drift: return drift;
        case EngineKind::Tree: return tree;
        default: return *vmp_family(e->kind);
    }
}

// rxhip_set_covariance_mode(1): the per-chain covariance array of a shared-model batch is written when somebody needs it
static rxhip_status ensure_cov(rxhip_engine* e) {
    if (!e || !e->cov_pending) return RXHIP_OK;
    SET_DEVICE(e);
    SplitParams sq{};
    sq.p.T = e->T; sq.p.S = e->S; sq.p.d_out = e->d; sq.p.cov = e->d_cov; sq.p.fe_part = nullptr;
    sq.vstab = e->d_vstab;
    hipLaunchKernelGGL(kd_split_broadcast, dim3(2048), dim3(256), 0, e->stream, sq, (long long)e->n_chains, 0, 1);
    HIPCHK(e, hipGetLastError());
    e->cov_pending = false;
    e->cov_current = true;
    e->cov_writes += 1;
    return RXHIP_OK;
}
rxhip_status rxhip_set_covariance_mode(rxhip_engine* e, int32_t mode) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (mode != 0 && mode != 1) return fail(e, RXHIP_ERR_BADARG, "set_covariance_mode: mode must be 0 (every sweep) or 1 (on request)");
    if (rxhip_status st = ensure_cov(e)) return st;
    e->cov_mode = mode;
    e->cov_current = false;   // the documented way to force a rewrite (a caller that wrote through rxhip_get_marginals_device): one sweep's stores
    return RXHIP_OK;
}
rxhip_status rxhip_get_covariance_writes(rxhip_engine* e, uint64_t* n) {
    TREE_GUARD(e);
    if (!e || !n) return RXHIP_ERR_BADARG;
    if (e->kind != EngineKind::Lgssm) return fail(e, RXHIP_ERR_UNSUPPORTED, "get_covariance_writes: not a state-space engine");
    *n = e->cov_writes;
    return RXHIP_OK;
}
rxhip_status rxhip_set_fixed_point_exits(rxhip_engine* e, int32_t enabled) {
    TREE_GUARD(e);   // (the executor has no such exits: every rule of its schedule is evaluated)
    if (!e) return RXHIP_ERR_BADARG;
    if (enabled != 0 && enabled != 1) return fail(e, RXHIP_ERR_BADARG, "set_fixed_point_exits: 0 (every recursion in full) or 1 (default)");
    e->full_recursions = enabled == 0;
    e->cov_current = false;   // (the shared-model tables keep their own convergence tests, so the bits would be the same: one sweep's stores for a rule without exceptions)
    return RXHIP_OK;
}
rxhip_status rxhip_sync(rxhip_engine* e) {
    if (!e) return RXHIP_ERR_BADARG;
    if (e->tree) return rxhip::tree::sync(e->tree, e->err);
    SET_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (rxhip_status pst = prof_drain(e, true)) return pst;
    int st = 0;
    HIPCHK(e, hipMemcpy(&st, e->d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) {
        HIPCHK(e, hipMemset(e->d_status, 0, sizeof(int)));
        if (st & ST_NLSSM_NONFINITE) {   // before ST_NOT_POSDEF: the lanes of other series may have raised that one in the same run, the first cause is this
            unsigned long long w = 0;
            HIPCHK(e, hipMemcpy(&w, e->nl.d_where, sizeof w, hipMemcpyDeviceToHost));
            return fail(e, RXHIP_ERR_NONFINITE_FE, "nlssm: f, its Jacobian or the predicted moments are not finite at step %llu of series %llu (counted from 0; the first "
                                                   "such event): no result of this run is valid (device flags 0x%x)", w >> 32, w & 0xffffffffull, st);
        }
        if (st & ST_NOT_POSDEF)
            return fail(e, RXHIP_ERR_NOT_POSDEF, "a covariance / precision block lost positive definiteness on device");
        if (st & ST_HMM_UNDERFLOW)
            return fail(e, RXHIP_ERR_NONFINITE_FE, "hmm: a normaliser of the forward–backward sweep underflowed (at or below 1e-200, or not finite): the counts are too "
                                                   "small for this sweep, no result of this run is valid (device flags 0x%x)", st);
        return fail(e, RXHIP_ERR_NONFINITE_FE, "free energy is NaN or Inf (device flags 0x%x)", st);
    }
    return RXHIP_OK;
}

rxhip_status rxhip_run(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (e && e->tree) {   // (synchronous: the drivers read the results immediately, src/inference/batch.jl:415)
        e->err.clear();
        return rxhip::tree::run(e->tree, iterations, want_fe, e->err);
    }
    rxhip_status st = rxhip_run_async(e, iterations, want_fe);
    if (st) return st;
    return rxhip_sync(e);
}

rxhip_status rxhip_lgssm_infer(rxhip_engine* e, const double* y, size_t n, int32_t iterations, int32_t want_fe, int32_t filtering,
                               double* mean, double* cov, double* fe_per_chain) {
    TREE_GUARD(e);
    TREE_GUARD(e);
    if (!e || !y) return RXHIP_ERR_BADARG;
    if (e->kind != EngineKind::Lgssm) return fail(e, RXHIP_ERR_BADARG, "infer: not a state-space engine");
    const size_t C = (size_t)e->n_chains, ny = (size_t)e->T * C * e->dy, nm = (size_t)e->Tout() * C * e->d, nc = nm * e->d;
    if (n != ny) return fail(e, RXHIP_ERR_BADARG, "infer: expected %zu doubles, got %zu", ny, n);
    // one staging block: y | the span of the results as it lies in the arena (status word | mean | cov | fe per chain, each 256-byte aligned:
    // ArenaPlan::zeroed_last / plain_first) or, for engines whose results are not adjacent, the same four pieces one after the other
    const char* const sp0 = reinterpret_cast<const char*>(e->d_status);
    const bool span = e->in_arena(e->d_status) && e->in_arena(e->d_mean) && e->in_arena(e->d_cov) && e->in_arena(e->d_fe_chain) &&
                      reinterpret_cast<const char*>(e->d_mean) == sp0 + 256 &&
                      reinterpret_cast<const char*>(e->d_cov) == reinterpret_cast<const char*>(e->d_mean) + ArenaPlan::al(sizeof(double) * nm) &&
                      reinterpret_cast<const char*>(e->d_fe_chain) == reinterpret_cast<const char*>(e->d_cov) + ArenaPlan::al(sizeof(double) * nc);
    const size_t total = ny + nm + nc + C + 1 + (span ? 4 * 32 : 0);
    // Larger problems gain nothing from fewer round trips and lose on the extra pass through the staging block (measured, d = 2:
    // T = 10⁴, 0.65 MB: 0.345 against 0.362 ms; T = 2.5·10⁴, 1.6 MB: 0.93 against 0.53): they take the plain sequence.
    if (sizeof(double) * total > ((size_t)512 << 10) || !e->d_y || !e->own_y) {
        rxhip_status st = rxhip_set_data(e, RXHIP_VAR_Y, y, n, RXHIP_LAYOUT_TIME_CHAIN);
        if (!st) st = filtering ? rxhip_run_filter(e, want_fe) : rxhip_run(e, iterations, want_fe);
        if (!st && (mean || cov)) st = rxhip_get_marginals(e, RXHIP_VAR_X, mean, cov, RXHIP_LAYOUT_TIME_CHAIN);
        if (!st && fe_per_chain && want_fe) st = rxhip_get_free_energy_per_chain(e, fe_per_chain);
        return st;
    }
    SET_DEVICE(e);
    if (e->h_io && e->h_io_bytes < sizeof(double) * total) { pinned_release(e->h_io, e->h_io_bytes); e->h_io = nullptr; }
    if (!e->h_io) {
        e->h_io = pinned_acquire(sizeof(double) * total, &e->h_io_bytes);
        if (!e->h_io) return fail(e, RXHIP_ERR_HIP, "infer: pinned staging allocation failed");
    }
    double *hy = e->h_io, *hm, *hc, *hf;
    int* hs;
    if (span) {
        char* hsp = reinterpret_cast<char*>(hy + ny);
        hs = reinterpret_cast<int*>(hsp);
        hm = reinterpret_cast<double*>(hsp + 256);
        hc = reinterpret_cast<double*>(hsp + 256 + ArenaPlan::al(sizeof(double) * nm));
        hf = reinterpret_cast<double*>(hsp + 256 + ArenaPlan::al(sizeof(double) * nm) + ArenaPlan::al(sizeof(double) * nc));
    } else {
        hm = hy + ny; hc = hm + nm; hf = hc + nc;
        hs = reinterpret_cast<int*>(hf + C);
    }
    std::memcpy(hy, y, sizeof(double) * ny);
    HIPCHK(e, hipMemcpyAsync(e->d_y, hy, sizeof(double) * ny, hipMemcpyHostToDevice, e->stream));
    if (e->d_nu) hipLaunchKernelGGL(k_shift_rows, dim3(2048), dim3(256), 0, e->stream, e->d_y, (const double*)e->d_nu, e->T, e->n_chains, e->dy, -1.0, e->off_chain ? 1 : 0);
    e->have_data = true;
    if (rxhip_status st = run_impl(e, filtering ? 1 : iterations, want_fe, filtering != 0)) return st;
    if (cov) { if (rxhip_status stc = ensure_cov(e)) return stc; }
    if (span) {   // everything the caller reads, in one copy (a copy command costs more than its 160 KB: four of them were a tenth of the call)
        const size_t bytes = (size_t)(reinterpret_cast<const char*>(e->d_fe_chain + C) - sp0);
        HIPCHK(e, hipMemcpyAsync(hs, e->d_status, bytes, hipMemcpyDeviceToHost, e->stream));
    } else {
        if (mean) HIPCHK(e, hipMemcpyAsync(hm, e->d_mean, sizeof(double) * nm, hipMemcpyDeviceToHost, e->stream));
        if (cov) HIPCHK(e, hipMemcpyAsync(hc, e->d_cov, sizeof(double) * nc, hipMemcpyDeviceToHost, e->stream));
        if (fe_per_chain && want_fe) HIPCHK(e, hipMemcpyAsync(hf, e->d_fe_chain, sizeof(double) * C, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipMemcpyAsync(hs, e->d_status, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));  // the one synchronisation of the call
    if (rxhip_status pst = prof_drain(e, true)) return pst;
    if (*hs) {
        HIPCHK(e, hipMemset(e->d_status, 0, sizeof(int)));
        if (*hs & ST_NOT_POSDEF) return fail(e, RXHIP_ERR_NOT_POSDEF, "a covariance / precision block lost positive definiteness on device");
        return fail(e, RXHIP_ERR_NONFINITE_FE, "free energy is NaN or Inf (device flags 0x%x)", *hs);
    }
    if (mean) std::memcpy(mean, hm, sizeof(double) * nm);
    if (cov) std::memcpy(cov, hc, sizeof(double) * nc);
    if (fe_per_chain && want_fe) std::memcpy(fe_per_chain, hf, sizeof(double) * C);
    return RXHIP_OK;
}

rxhip_status rxhip_get_marginals_device(rxhip_engine* e, int32_t var_id, const double** mean_dev,
                                        const double** cov_dev) {
    TREE_GUARD(e);
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (var_id != RXHIP_VAR_X || !family_of(e).has_x) return fail(e, RXHIP_ERR_BADARG, "get_marginals: variable %d is not random", var_id);
    if (!e->ran) return fail(e, RXHIP_ERR_STATE, "get_marginals: no run yet");
    if (rxhip_status stc = ensure_cov(e)) return stc;   // covariance mode 1: the per-chain array is written now
    if (mean_dev) *mean_dev = e->d_mean;
    if (cov_dev) *cov_dev = e->d_cov;
    return RXHIP_OK;
}

static rxhip_status copy_out(rxhip_engine* e, const double* dsrc, double* host, int k, int32_t layout, long long rows = -1) {
    if (rows < 0) rows = e->T;
    const size_t n = (size_t)rows * e->n_chains * k;
    if (layout == RXHIP_LAYOUT_TIME_CHAIN || e->n_chains == 1) {
        HIPCHK(e, hipMemcpy(host, dsrc, sizeof(double) * n, hipMemcpyDeviceToHost));
        return RXHIP_OK;
    }
    DevTmp tmp_guard;
    HIPCHK(e, hipMalloc(&tmp_guard.p, sizeof(double) * n));
    double* tmp = (double*)tmp_guard.p;
    // [T][chain][k] -> [chain][T][k]
    hipLaunchKernelGGL(k_transpose_rows, dim3(2048), dim3(256), 0, e->stream, dsrc, tmp, rows, e->n_chains, k);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(host, tmp, sizeof(double) * n, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}

rxhip_status rxhip_hgf_get_history(rxhip_engine* e, double* z_mean, double* z_var, double* x_mean, double* x_var,
                                   int32_t layout) {
    TREE_GUARD(e);
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Hgf) return RXHIP_ERR_BADARG;
    if (!e->ran) return fail(e, RXHIP_ERR_STATE, "get_history: no run yet");
    if (layout != RXHIP_LAYOUT_TIME_CHAIN && layout != RXHIP_LAYOUT_CHAIN_TIME)
        return fail(e, RXHIP_ERR_BADARG, "get_history: unknown layout %d", layout);
    SET_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const size_t n = (size_t)e->T * e->n_chains;
    double* outs[4] = {z_mean, z_var, x_mean, x_var};
    for (int q = 0; q < 4; ++q) {
        rxhip_status st;
        if (outs[q] && (st = copy_out(e, e->h.d_out + q * n, outs[q], 1, layout))) return st;
    }
    return RXHIP_OK;
}

rxhip_status rxhip_get_marginals(rxhip_engine* e, int32_t var_id, double* mean, double* cov, int32_t layout) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (var_id != RXHIP_VAR_X || !family_of(e).has_x) return fail(e, RXHIP_ERR_BADARG, "get_marginals: variable %d is not random", var_id);
    if (!e->ran) return fail(e, RXHIP_ERR_STATE, "get_marginals: no run yet");
    if (layout != RXHIP_LAYOUT_TIME_CHAIN && layout != RXHIP_LAYOUT_CHAIN_TIME)
        return fail(e, RXHIP_ERR_BADARG, "get_marginals: unknown layout %d", layout);
    SET_DEVICE(e);
    if (cov) { if (rxhip_status stc = ensure_cov(e)) return stc; }   // covariance mode 1: the per-chain array is written now
    HIPCHK(e, hipStreamSynchronize(e->stream));
    rxhip_status st;
    // small results (the reference's own benchmark sizes): mean and covariance sit next to each other in the arena, so ONE
    // device-to-host copy of the span serves both — a synchronous hipMemcpy costs ≈12 µs whatever its size
    const size_t nm = (size_t)e->Tout() * e->n_chains * e->d, nc = nm * e->d;
    const bool same_layout = layout == RXHIP_LAYOUT_TIME_CHAIN || e->n_chains == 1;
    if (mean && cov && same_layout && e->in_arena(e->d_mean) && e->in_arena(e->d_cov) && e->d_cov > e->d_mean &&
        (size_t)((e->d_cov + nc) - e->d_mean) <= ((size_t)1 << 17)) {
        const size_t span = (size_t)((e->d_cov + nc) - e->d_mean);
        std::vector<double> stage(span);
        HIPCHK(e, hipMemcpy(stage.data(), e->d_mean, sizeof(double) * span, hipMemcpyDeviceToHost));
        std::memcpy(mean, stage.data(), sizeof(double) * nm);
        std::memcpy(cov, stage.data() + (e->d_cov - e->d_mean), sizeof(double) * nc);
        return RXHIP_OK;
    }
    if (mean && (st = copy_out(e, e->d_mean, mean, e->d, layout, e->Tout()))) return st;
    if (cov && (st = copy_out(e, e->d_cov, cov, e->d * e->d, layout, e->Tout()))) return st;
    return RXHIP_OK;
}

rxhip_status rxhip_get_predictions(rxhip_engine* e, int32_t var_id, double* mean, double* cov, int32_t layout) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (var_id != RXHIP_VAR_Y || e->kind != EngineKind::Lgssm) return fail(e, RXHIP_ERR_BADARG, "get_predictions: variable %d is not a data variable of a state-space engine", var_id);
    if (!e->ran || e->last_filter) return fail(e, RXHIP_ERR_STATE, "get_predictions: needs a smoothing run (rxhip_run) first");
    if (layout != RXHIP_LAYOUT_TIME_CHAIN && layout != RXHIP_LAYOUT_CHAIN_TIME) return fail(e, RXHIP_ERR_BADARG, "get_predictions: unknown layout %d", layout);
    SET_DEVICE(e);
    if (rxhip_status stc = ensure_cov(e)) return stc;
    const size_t rows = (size_t)e->Tout() * e->n_chains, dy = (size_t)e->dy;
    if (e->dense) {  // any d, dy ≤ 64: observation-space form, one workgroup per (chain, time index)
        // 133 KB of dynamic LDS at d = dy = 64 (the kernel also holds a few bytes of static LDS: not the full 160 KB)
        once_per_device(3, e->device, [] { (void)hipFuncSetAttribute((const void*)k_predict_generic, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024); });
        DevTmp tmp_guard;
        HIPCHK(e, hipMalloc(&tmp_guard.p, sizeof(double) * rows * (dy + dy * dy)));
        double* tmp = (double*)tmp_guard.p;
        GenericParams gp{};
        gp.T = e->T; gp.H = e->H; gp.n_chains = e->n_chains; gp.d = e->d; gp.dy = e->dy; gp.y = e->d_y; gp.mean = e->d_mean; gp.cov = e->d_cov;
        gp.user = e->d_user; gp.chain_model = e->d_chain_model; gp.step_model = e->d_step_model; gp.pmean = tmp; gp.pcov = tmp + rows * dy; gp.status = e->d_status;
        gp.mu = e->d_mu; gp.nu = e->d_nu; gp.off_chain = e->off_chain ? 1 : 0;
        hipLaunchKernelGGL(k_predict_generic, dim3((unsigned)rows), dim3(256), generic_predict_lds(e->d, e->dy), e->stream, gp);
        rxhip_status st = RXHIP_OK;
        if (hipGetLastError() != hipSuccess) st = fail(e, RXHIP_ERR_HIP, "prediction kernel launch failed");
        if (!st) st = rxhip_sync(e);
        if (!st && mean) st = copy_out(e, gp.pmean, mean, e->dy, layout, e->Tout());
        if (!st && cov) st = copy_out(e, gp.pcov, cov, e->dy * e->dy, layout, e->Tout());
        return st;
    }
    if (!e->vt) return fail(e, RXHIP_ERR_UNSUPPORTED, "predictions: no schedule for this shape");
    if (!e->d_bq) {
        HIPCHK(e, hipMalloc(&e->d_bq, sizeof(double) * e->h_bq.size()));
        HIPCHK(e, hipMemcpy(e->d_bq, e->h_bq.data(), sizeof(double) * e->h_bq.size(), hipMemcpyHostToDevice));
    }
    DevTmp tmp_guard;
    HIPCHK(e, hipMalloc(&tmp_guard.p, sizeof(double) * rows * (dy + dy * dy)));
    double* tmp = (double*)tmp_guard.p;
    PredictParams pp{};
    pp.T = e->T; pp.H = e->H; pp.n_chains = e->n_chains; pp.y = e->d_y; pp.mean = e->d_mean; pp.cov = e->d_cov; pp.cst = e->d_cst;
    pp.bq = e->d_bq; pp.chain_model = e->d_chain_model; pp.step_model = e->d_step_model; pp.pmean = tmp; pp.pcov = tmp + rows * dy; pp.status = e->d_status;
    pp.mu = e->d_mu; pp.nu = e->d_nu; pp.off_chain = e->off_chain ? 1 : 0;
    e->vt->predict(pp, e->stream);
    rxhip_status st = RXHIP_OK;
    if (hipGetLastError() != hipSuccess) st = fail(e, RXHIP_ERR_HIP, "prediction kernel launch failed");
    if (!st) st = rxhip_sync(e);  // also reports a leave-one-out precision that is not positive definite
    if (!st && mean) st = copy_out(e, pp.pmean, mean, e->dy, layout, e->Tout());
    if (!st && cov) st = copy_out(e, pp.pcov, cov, e->dy * e->dy, layout, e->Tout());
    return st;
}

rxhip_status rxhip_get_node_marginals(rxhip_engine* e, int32_t node_type, double* mean, double* cov, int32_t layout) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (node_type != RXHIP_NODE_MVNORMAL_MEAN_COV || e->kind != EngineKind::Lgssm)
        return fail(e, RXHIP_ERR_BADARG, "get_node_marginals: node-local joints exist for the transition nodes of a state-space engine");
    if (!e->ran || e->last_filter) return fail(e, RXHIP_ERR_STATE, "get_node_marginals: needs a smoothing run (rxhip_run) first");
    if (!e->dense && !e->vt) return fail(e, RXHIP_ERR_UNSUPPORTED, "node-local joints: no device schedule for this shape");
    if (layout != RXHIP_LAYOUT_TIME_CHAIN && layout != RXHIP_LAYOUT_CHAIN_TIME) return fail(e, RXHIP_ERR_BADARG, "get_node_marginals: unknown layout %d", layout);
    if (e->T < 2) return RXHIP_OK;  // a single time step has no transition node between observed states
    SET_DEVICE(e);
    if (rxhip_status stc = ensure_cov(e)) return stc;
    const size_t rows = (size_t)(e->T - 1) * e->n_chains, d2 = 2 * (size_t)e->d;
    DevTmp tmp_guard;
    HIPCHK(e, hipMalloc(&tmp_guard.p, sizeof(double) * rows * (d2 + d2 * d2)));
    double* tmp = (double*)tmp_guard.p;
    if (e->dense) {
        // any d ≤ 64: Cov(x[t], x[t+1] | y) = G_t V_s(t+1) is what the joints need beyond the posteriors, and no schedule of the
        // MFMA path keeps it.  The sequential kernels recompute the sweep into scratch arrays with that product kept
        // (gseq_kernels.hpp: one workgroup per chain) — a getter, not a hot path; the engine's own posteriors stay as they are.
        const size_t C = (size_t)e->n_chains, T = (size_t)e->T, d = (size_t)e->d;
        const size_t nm = T * C * d, nc = T * C * d * d, nx = (T - 1) * C * d * d;
        double* scr = nullptr;
        if (hipMalloc(&scr, sizeof(double) * (nm + nc + nx)) != hipSuccess) {
            return fail(e, RXHIP_ERR_HIP, "get_node_marginals: hipMalloc of %zu bytes of scratch failed", sizeof(double) * (nm + nc + nx));
        }
        once_per_device(0, e->device, [] {
            (void)hipFuncSetAttribute((const void*)k_gseq_forward, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
            (void)hipFuncSetAttribute((const void*)k_gseq_backward, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        });
        once_per_device(4, e->device, [] { (void)hipFuncSetAttribute((const void*)k_joint_generic, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024); });
        GseqParams gq{};
        gq.T = e->T; gq.n_chains = e->n_chains; gq.d = e->d; gq.dy = e->dy; gq.ptt = e->ptt; gq.fe = 0; gq.y = e->d_y;
        gq.mean = scr; gq.cov = scr + nm; gq.cross = scr + nm + nc; gq.user = e->d_user; gq.prior = e->d_prior;
        gq.chain_model = e->d_chain_model; gq.step_model = e->d_step_model; gq.fe_part = nullptr; gq.status = e->d_status;
        // After a sweep of the information-form kernels (one chain per tile, no model / data split) the smoother gains are still in the
        // records: the cross-covariances are one product per time index.  Otherwise: the sequential re-run.
        const bool from_records = e->records_hold_gains && !e->hooks.joints_gseq;
        if (from_records) {
            DenseParams cp{};
            const int nt = e->mseg ? e->m_nt : e->nt;
            cp.T = e->T; cp.n_chains = e->n_chains; cp.d = 16 * nt; cp.d_out = e->d; cp.filt = e->d_filt; cp.cov = e->d_cov;
            cp.L = e->L > 0 ? e->L : 1; cp.S = e->S; cp.mseg = e->mseg ? 1 : 0; cp.step_model = e->d_step_model;   // (where a frozen stretch's matrices live: kd_forward_info FZ_SLOT)
            const dim3 gr((unsigned)((e->T - 1) * e->n_chains));
            dense_vt(nt)->cross_from_records(cp, gq.cross, gr, e->stream);
        } else {
        const size_t lds = gseq_lds_bytes(e->d, e->dy);
        hipLaunchKernelGGL(k_gseq_forward, dim3((unsigned)e->n_chains), dim3(256), lds, e->stream, gq);
        hipLaunchKernelGGL(k_gseq_backward, dim3((unsigned)e->n_chains), dim3(256), lds, e->stream, gq);
        }
        JointParams jp{};
        jp.T = e->T; jp.n_chains = e->n_chains; jp.d = e->d; jp.dy = e->dy; jp.mean = e->d_mean; jp.cov = e->d_cov; jp.cross = gq.cross;
        jp.user = e->d_user; jp.chain_model = e->d_chain_model; jp.step_model = e->d_step_model; jp.cx = e->d_cx; jp.off_chain = e->off_chain ? 1 : 0;
        jp.jmean = tmp; jp.jcov = tmp + rows * d2;
        hipLaunchKernelGGL(k_joint_generic, dim3((unsigned)rows), dim3(256), joint_lds_bytes(e->d), e->stream, jp);
        rxhip_status st = RXHIP_OK;
        if (hipGetLastError() != hipSuccess) st = fail(e, RXHIP_ERR_HIP, "joint-marginal kernel launch failed");
        if (!st) st = rxhip_sync(e);
        if (!st && mean) st = copy_out(e, jp.jmean, mean, (int)d2, layout, e->T - 1);
        if (!st && cov) st = copy_out(e, jp.jcov, cov, (int)(d2 * d2), layout, e->T - 1);
        (void)hipFree(scr);
        return st;
    }
    PredictParams pp{};
    pp.T = e->T; pp.H = 0; pp.n_chains = e->n_chains; pp.mean = e->d_mean; pp.cov = e->d_cov; pp.cst = e->d_cst;
    pp.chain_model = e->d_chain_model; pp.step_model = e->d_step_model; pp.status = e->d_status;
    pp.filt = e->uniform ? nullptr : e->d_filt; pp.vtab = e->d_vtab;
    pp.tinv_tc = e->records_tinv ? e->d_elem : nullptr; pp.L = e->L;
    pp.jmean = tmp; pp.jcov = tmp + rows * d2; pp.cx = e->d_cx; pp.off_chain = e->off_chain ? 1 : 0;
    e->vt->joint(pp, e->stream);
    rxhip_status st = RXHIP_OK;
    if (hipGetLastError() != hipSuccess) st = fail(e, RXHIP_ERR_HIP, "joint-marginal kernel launch failed");
    if (!st) st = rxhip_sync(e);
    if (!st && mean) st = copy_out(e, pp.jmean, mean, (int)d2, layout, e->T - 1);
    if (!st && cov) st = copy_out(e, pp.jcov, cov, (int)(d2 * d2), layout, e->T - 1);
    return st;
}

rxhip_status rxhip_get_free_energy(rxhip_engine* e, double* per_iteration) {
    if (!e || !per_iteration) return RXHIP_ERR_BADARG;
    if (e->tree) return rxhip::tree::get_free_energy(e->tree, per_iteration, e->err);
    if (!e->ran || !e->last_want_fe) return fail(e, RXHIP_ERR_STATE, "free energy was not requested in the last run");
    SET_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(per_iteration, fe_total_of(e), sizeof(double) * e->last_iterations,
                        hipMemcpyDeviceToHost));
    return RXHIP_OK;
}
rxhip_status rxhip_get_free_energy_per_chain(rxhip_engine* e, double* per_chain) {
    if (!e || !per_chain) return RXHIP_ERR_BADARG;
    if (e->tree) return rxhip::tree::get_free_energy_per_replica(e->tree, per_chain, e->err);
    if (e->kind == EngineKind::Mixture) return fail(e, RXHIP_ERR_BADARG, "per-chain free energy is not defined for the mixture engine");
    if (!e->ran || !e->last_want_fe) return fail(e, RXHIP_ERR_STATE, "free energy was not requested in the last run");
    SET_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(per_chain, e->d_fe_chain, sizeof(double) * e->n_chains, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}
rxhip_status rxhip_get_free_energy_device(rxhip_engine* e, double** fe_dev) {
    TREE_GUARD(e);
    if (!e || !fe_dev) return RXHIP_ERR_BADARG;
    if (!e->ran || !e->last_want_fe) return fail(e, RXHIP_ERR_STATE, "free energy was not requested in the last run");
    *fe_dev = fe_total_of(e) + (e->last_iterations - 1);
    return RXHIP_OK;
}

rxhip_status rxhip_copy_free_energy_to_device(rxhip_engine* e, double* dst_dev) {
    TREE_GUARD(e);
    if (!e || !dst_dev) return RXHIP_ERR_BADARG;
    if (!e->ran || !e->last_want_fe) return fail(e, RXHIP_ERR_STATE, "free energy was not requested in the last run");
    SET_DEVICE(e);
    HIPCHK(e, hipMemcpyAsync(dst_dev, fe_total_of(e) + (e->last_iterations - 1), sizeof(double),
                             hipMemcpyDeviceToDevice, e->stream));
    return RXHIP_OK;
}

rxhip_status rxhip_counters(rxhip_engine* e, uint64_t* rule_calls, uint64_t* products, uint64_t* marginals) {
    if (!e) return RXHIP_ERR_BADARG;
    if (e->tree) { rxhip::tree::counters(e->tree, rule_calls, products, marginals); return RXHIP_OK; }
    if (rule_calls) *rule_calls = e->rule_calls;
    if (products) *products = e->products;
    if (marginals) *marginals = e->marginals;
    return RXHIP_OK;
}

rxhip_status rxhip_set_profiling(rxhip_engine* e, int32_t enabled) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    e->profiling = enabled != 0;
    if (e->profiling) {   // the events a profiled run needs (64 pending pairs at most) exist before it starts: no hipEventCreate inside a timed region
        SET_DEVICE(e);
        while (e->pool.size() + 2 * e->pending.size() < 130) {
            hipEvent_t ev;
            HIPCHK(e, hipEventCreate(&ev));
            e->pool.push_back(ev);
        }
    }
    return RXHIP_OK;
}
rxhip_status rxhip_get_kernel_times(rxhip_engine* e, double* ms_avg, uint64_t* launches) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    for (int k = 0; k < RXHIP_K_COUNT; ++k) {
        if (ms_avg) ms_avg[k] = e->k_n[k] ? e->k_ms[k] / (double)e->k_n[k] : 0.0;
        if (launches) launches[k] = e->k_n[k];
    }
    return RXHIP_OK;
}
rxhip_status rxhip_get_create_stages(rxhip_engine* e, double* ms4) {
    TREE_GUARD(e);
    if (!e || !ms4) return RXHIP_ERR_BADARG;
    for (int q = 0; q < STAGE_COUNT; ++q) ms4[q] = e->stage_ms[q];
    return RXHIP_OK;
}
rxhip_status rxhip_get_mean_checkpoint_stride(rxhip_engine* e, int32_t* K) {
    TREE_GUARD(e);
    if (!e || !K) return RXHIP_ERR_BADARG;
    *K = e->ck_log2 ? (int32_t)1 << e->ck_log2 : 0;
    return RXHIP_OK;
}
rxhip_status rxhip_get_sweep_waves(rxhip_engine* e, int32_t* forward, int32_t* backward) {
    TREE_GUARD(e);
    if (!e || !forward || !backward) return RXHIP_ERR_BADARG;
    *forward = e->ck_log2 ? e->sweep_waves_fwd : 0;
    *backward = e->ck_log2 ? e->sweep_waves_bwd : 0;
    return RXHIP_OK;
}
rxhip_status rxhip_get_model_tables_ms(rxhip_engine* e, double* ms) {
    TREE_GUARD(e);
    if (!e || !ms) return RXHIP_ERR_BADARG;
    *ms = 0.0;
    if (!e->ev_tab1) return RXHIP_OK;
    SET_DEVICE(e);
    HIPCHK(e, hipEventSynchronize(e->ev_tab1));
    float f = 0.0f;
    HIPCHK(e, hipEventElapsedTime(&f, e->ev_tab0, e->ev_tab1));
    *ms = (double)f;
    return RXHIP_OK;
}
rxhip_status rxhip_reset_kernel_times(rxhip_engine* e) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    for (int k = 0; k < RXHIP_K_COUNT; ++k) {
        e->k_ms[k] = 0.0;
        e->k_n[k] = 0;
    }
    return RXHIP_OK;
}
rxhip_status rxhip_get_stream(rxhip_engine* e, void** stream) {
    if (!e || !stream) return RXHIP_ERR_BADARG;
    if (e->tree) { *stream = rxhip::tree::stream_of(e->tree); return RXHIP_OK; }
    *stream = (void*)e->stream;
    return RXHIP_OK;
}
rxhip_status rxhip_get_schedule(rxhip_engine* e, int32_t* segments, int64_t* segment_len) {
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (e->kind == EngineKind::Mixture) {
        if (segments) *segments = e->g.nblocks;
        if (segment_len) *segment_len = 256;
        return RXHIP_OK;
    }
    if (segments) *segments = e->mseg ? e->mS : e->S;          // masked / per-step engines: the schedule of dense_mseg_kernels.hpp
    if (segment_len) *segment_len = e->mseg ? e->mL : e->L;
    return RXHIP_OK;
}


rxhip_status rxhip_get_marginals_chains(rxhip_engine* e, int32_t var_id, const int64_t* chains, int64_t n, double* mean,
                                        double* cov) {
    TREE_GUARD(e);
    TREE_GUARD(e);
    if (!e) return RXHIP_ERR_BADARG;
    if (var_id != RXHIP_VAR_X || !family_of(e).has_x) return fail(e, RXHIP_ERR_BADARG, "get_marginals_chains: variable %d is not random", var_id);
    if (!e->ran) return fail(e, RXHIP_ERR_STATE, "get_marginals_chains: no run yet");
    if (!chains || n <= 0) return fail(e, RXHIP_ERR_BADARG, "get_marginals_chains: empty chain list");
    for (int64_t i = 0; i < n; ++i)
        if (chains[i] < 0 || chains[i] >= e->n_chains) return fail(e, RXHIP_ERR_BADARG, "get_marginals_chains: chain %lld out of range", (long long)chains[i]);
    SET_DEVICE(e);
    if (cov) { if (rxhip_status stc = ensure_cov(e)) return stc; }
    const size_t nm = (size_t)n * e->Tout() * e->d, nc = nm * e->d;
    DevTmp tmp_guard;
    HIPCHK(e, hipMalloc(&tmp_guard.p, sizeof(long long) * (size_t)n + sizeof(double) * (nm + nc)));
    char* tmp = (char*)tmp_guard.p;
    double* g_mean = (double*)tmp;
    double* g_cov = g_mean + nm;
    long long* d_ch = (long long*)(g_cov + nc);
    rxhip_status st = RXHIP_OK;
    auto chk = [&](hipError_t err, const char* what) {
        if (err != hipSuccess && !st) st = fail(e, RXHIP_ERR_HIP, "%s failed: %s", what, hipGetErrorString(err));
    };
    static_assert(sizeof(long long) == sizeof(int64_t), "chain ids are 64-bit");
    chk(hipMemcpyAsync(d_ch, chains, sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, e->stream), "chain list upload");
    if (!st && mean) hipLaunchKernelGGL(k_gather_chains, dim3(1024), dim3(256), 0, e->stream, (const double*)e->d_mean, g_mean, (const long long*)d_ch, (long long)n, e->Tout(), e->n_chains, e->d);
    if (!st && cov) hipLaunchKernelGGL(k_gather_chains, dim3(1024), dim3(256), 0, e->stream, (const double*)e->d_cov, g_cov, (const long long*)d_ch, (long long)n, e->Tout(), e->n_chains, e->d * e->d);
    chk(hipGetLastError(), "gather launch");
    chk(hipStreamSynchronize(e->stream), "gather");
    if (!st && mean) chk(hipMemcpy(mean, g_mean, sizeof(double) * nm, hipMemcpyDeviceToHost), "copy of means");
    if (!st && cov) chk(hipMemcpy(cov, g_cov, sizeof(double) * nc, hipMemcpyDeviceToHost), "copy of covariances");
    return st;
}

// ------------------------------------------------------------------------------------------
// Cross-GPU exchange over RCCL (xGMI).  librccl is opened on first use, not linked: single-GPU hosts never need it, and
// a process that already carries an RCCL (torch) keeps exactly that one.
}  // extern "C"
