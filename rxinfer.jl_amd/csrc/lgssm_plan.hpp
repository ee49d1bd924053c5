// lgssm_plan.hpp — which schedule a linear-Gaussian state-space engine takes, decided on the host: the test hooks, read ONCE per engine, and the
// pure functions rxhip_lgssm_create fills the engine's schedule fields from.  No HIP: tests/test_lgssm_plan_cpu.py compiles this header with the
// host compiler and holds the segmentation to a table recorded on the device (tests/golden/lgssm_schedules.json).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

namespace rxhip {
namespace plan {

// Every schedule hook of the state-space engines (include/rxhip.h "Environment"): X(type, field, default).  The list is the struct, the
// engine-pool key and the field loop of the test, so a hook added here is in all three.
#define RXHIP_SCHEDULE_HOOKS(X)                                                                                                        \
    X(int, one_pass, -1)                  /* RXHIP_ONE_PASS=0|1 (-1: by size) */                                                        \
    X(bool, one_segment, false)           /* RXHIP_ONE_SEGMENT */                                                                       \
    X(bool, backward_lanes, false)        /* RXHIP_BACKWARD_LANES */                                                                    \
    X(bool, mean_records, false)          /* RXHIP_MEAN_RECORDS=1 */                                                                    \
    X(int, mean_checkpoint, 0)            /* RXHIP_MEAN_CHECKPOINT=K as a number (0: not set); rxhip_lgssm_create validates it */        \
    X(Text, mean_checkpoint_text, Text{}) /* … and as written, for the error message */                                                  \
    X(bool, boundary_kernel, false)       /* RXHIP_BOUNDARY_KERNEL=1 */                                                                 \
    X(bool, small_sweep_off, false)       /* RXHIP_SMALL_SWEEP=0 */                                                                     \
    X(bool, elem_full, false)             /* RXHIP_ELEM_FULL */                                                                         \
    X(bool, noise_moments_pass, false)    /* RXHIP_NOISE_MOMENTS_PASS */                                                                \
    X(bool, no_pack, false)               /* RXHIP_NO_PACK */                                                                           \
    X(int, dense_split, -1)               /* RXHIP_DENSE_SPLIT=0|1 (-1: from four workgroups' worth of chains) */                       \
    X(bool, host_tables, false)           /* RXHIP_HOST_TABLES */                                                                       \
    X(bool, gseq, false)                  /* RXHIP_GSEQ */                                                                              \
    X(bool, stepm_gseq, false)            /* RXHIP_STEPM_GSEQ */                                                                        \
    X(bool, filter_gseq, false)           /* RXHIP_FILTER_GSEQ */                                                                       \
    X(bool, joints_gseq, false)           /* RXHIP_JOINTS_GSEQ */                                                                       \
    X(int, mseg_scan, 0)                  /* RXHIP_MSEG_SCAN: 1 sequential, 2 log (0: the cheaper one) */                               \
    X(bool, mseg_one_level, false)        /* RXHIP_MSEG_ONE_LEVEL */                                                                    \
    X(int, mseg_group, 0)                 /* RXHIP_MSEG_GROUP=g (0: by cost) */                                                         \
    X(unsigned long long, mseg_max_bytes, ~0ULL) /* RXHIP_MSEG_MAX_BYTES=n (all ones: no cap) */                                        \
    X(bool, wave8_off, false)             /* RXHIP_WAVE8=0 */                                                                           \
    X(bool, no_frozen, false)             /* RXHIP_NO_FROZEN */                                                                         \
    X(bool, cov_every_sweep, false)       /* RXHIP_COV_EVERY_SWEEP=1 */                                                                 \
    X(int, y_ring, 0)                     /* RXHIP_Y_RING=1 (0: not set, -1: any other value; rxhip_lgssm_create refuses it) */                 \
    X(int, sweep_waves, 0)                /* RXHIP_SWEEP_WAVES=1|2|4 (0: not set, -1: any other value; rxhip_lgssm_create refuses it) */

struct Text { char s[16] = {0}; };   // the first 15 characters of a hook's value

struct ScheduleHooks {
#define X(type, field, dflt) type field = dflt;
    RXHIP_SCHEDULE_HOOKS(X)
#undef X
    // The only reader of these variables.  `get` is launch_tables.hpp's hook_env in the library (nothing is read without RXHIP_TEST_HOOKS=1).
    template <class Get>
    static ScheduleHooks read(Get get) {
        ScheduleHooks h;
        auto set = [&](const char* n) { return get(n) != nullptr; };
        auto is0 = [&](const char* n) { const char* v = get(n); return v && std::atoi(v) == 0; };
        auto not0 = [&](const char* n) { const char* v = get(n); return v && std::atoi(v) != 0; };
        auto tri = [&](const char* n) { const char* v = get(n); return v ? (std::atoi(v) != 0 ? 1 : 0) : -1; };
        auto num = [&](const char* n) { const char* v = get(n); return v ? std::atoi(v) : 0; };
        h.one_pass = tri("RXHIP_ONE_PASS");
        h.one_segment = set("RXHIP_ONE_SEGMENT");
        h.backward_lanes = set("RXHIP_BACKWARD_LANES");
        h.mean_records = not0("RXHIP_MEAN_RECORDS");
        if (const char* v = get("RXHIP_MEAN_CHECKPOINT")) {
            h.mean_checkpoint = std::atoi(v);
            if (h.mean_checkpoint == 0) h.mean_checkpoint = -1;   // set, and not a stride: refused at creation like any other bad value
            std::strncpy(h.mean_checkpoint_text.s, v, sizeof h.mean_checkpoint_text.s - 1);
        }
        h.boundary_kernel = not0("RXHIP_BOUNDARY_KERNEL");
        h.small_sweep_off = is0("RXHIP_SMALL_SWEEP");
        h.elem_full = set("RXHIP_ELEM_FULL");
        h.noise_moments_pass = set("RXHIP_NOISE_MOMENTS_PASS");
        h.no_pack = set("RXHIP_NO_PACK");
        h.dense_split = tri("RXHIP_DENSE_SPLIT");
        h.host_tables = set("RXHIP_HOST_TABLES");
        h.gseq = set("RXHIP_GSEQ");
        h.stepm_gseq = set("RXHIP_STEPM_GSEQ");
        h.filter_gseq = set("RXHIP_FILTER_GSEQ");
        h.joints_gseq = set("RXHIP_JOINTS_GSEQ");
        if (const char* v = get("RXHIP_MSEG_SCAN")) h.mseg_scan = !std::strcmp(v, "sequential") ? 1 : !std::strcmp(v, "log") ? 2 : 0;
        h.mseg_one_level = set("RXHIP_MSEG_ONE_LEVEL");
        h.mseg_group = num("RXHIP_MSEG_GROUP");
        if (const char* v = get("RXHIP_MSEG_MAX_BYTES")) h.mseg_max_bytes = std::strtoull(v, nullptr, 10);
        h.wave8_off = is0("RXHIP_WAVE8");
        h.no_frozen = set("RXHIP_NO_FROZEN");
        h.cov_every_sweep = not0("RXHIP_COV_EVERY_SWEEP");
        if (const char* v = get("RXHIP_Y_RING")) h.y_ring = !std::strcmp(v, "1") ? 1 : -1;
        if (const char* v = get("RXHIP_SWEEP_WAVES")) h.sweep_waves = !std::strcmp(v, "1") ? 1 : !std::strcmp(v, "2") ? 2 : !std::strcmp(v, "4") ? 4 : -1;
        return h;
    }
    // the hooks' part of the engine-pool key: every field, by the list above
    void append_key(std::string& key) const {
#define X(type, field, dflt) key.append(reinterpret_cast<const char*>(&field), sizeof field);
        RXHIP_SCHEDULE_HOOKS(X)
#undef X
    }
};

// What the planner needs of a descriptor (rxhip_lgssm_desc) and of the kernel families: `dense` — the MFMA path (no d, dy ≤ 4 kernels for this shape)
struct Shape {
    int d = 0, dy = 0;
    long long T = 0, n_chains = 0;
    int n_models = 1;
    long long segments = 0;   // desc.segments: a request (0: the engine chooses)
    bool dense = false, allow_missing = false, step_model = false, chain_model = false;
};

// Static schedule flags of an engine
struct Flags {
    bool sequential = false, uniform = true, gseq = false, masked = false;
    int dpad = 0, nt = 0;     // dense path: d rounded up to a multiple of 16, tiles per side
    int pack = 1;             // 2: pairs of chains share a 16×16 tile
    long long wg_chains = 0;  // chains (or pairs) the kernels' grids run over
    int dyk = 0;              // observation dimension at kernel level
};
inline Flags static_flags(const Shape& s, const ScheduleHooks& hooks) {
    Flags f;
    f.dpad = s.dense ? (s.d + 15) / 16 * 16 : s.d;
    f.nt = f.dpad / 16;
    f.uniform = (s.n_models == 1);
    if (s.allow_missing) {
        // `missing` observations change the covariances per chain and per time index: no table of the time-parallel schedule
        // survives.  The chain runs as ONE segment (sequential in time, parallel over chains) on the per-chain-record kernels.
        if (s.dense) f.gseq = true;  // any d, dy ≤ 64: one workgroup per chain, sequential in time (gseq_kernels.hpp)
        f.masked = true;
        f.sequential = true;
        f.uniform = false;
    }
    if (s.step_model) {
        // time-varying A_t, P_t, B_t, Q_t: the tables of the time-parallel schedule assume one model along the chain
        if (s.dense) f.gseq = true;
        f.sequential = true;
        f.uniform = false;
    }
    // Per-chain models take the same table-free route: per-position gain tables PER MODEL were 256 B per lane and step of
    // streamed traffic (26 GB per sweep at C2 with n_models = n_chains — more than the observations and posteriors together);
    // computing the element in the lane costs less than reading it (measured: k_seg_aggregate 5.97 ms -> k_seg_elements)
    if (!s.dense && !f.uniform) f.sequential = true;
    // d ≤ 8: two chains per 16×16 tile (block-diagonal pair) instead of one chain padded to 16 — twice the chains per
    // workgroup for the same MFMA work.  Needs an even batch (the pair is formed from neighbours in memory).
    f.pack = (s.dense && !f.gseq && s.d <= 8 && s.dy <= 32 && s.n_chains % 2 == 0 && s.n_models == 1 && !hooks.no_pack) ? 2 : 1;
    f.wg_chains = s.n_chains / f.pack;
    f.dyk = s.dy * f.pack;
    return f;
}

// One model for at least four workgroups' worth of chains on the MFMA path: the matrices of the information-form smoother are computed
// once (model pass on one chain), every sweep is vectors only (d = 8 × 1024 chains × T = 1000: 1.86 -> 0.77 ms;
// d = 64 × 64 chains: 5.70 -> 1.92 ms).  RXHIP_DENSE_SPLIT=0/1 overrides (tests).
inline bool split_wanted(long long wg_chains, const ScheduleHooks& hooks) { return hooks.dense_split >= 0 ? hooks.dense_split != 0 : wg_chains >= 4; }

struct Segmentation {
    int S = 0;
    long long L = 1, Llast = 1;
    bool small_short = false;
};
// time segmentation: two (chain, segment) lanes per SIMD lane slot — 256 CUs × 4 SIMDs × 2 waves × 64 lanes.
// Once the forward message is stored compactly the backward kernel is issue-bound at one wave per SIMD
// (measured at C2: 4.7 ms with 64 segments, 3.9–4.0 ms with 128…512); the boundary scan is cheap.
// Dense (MFMA) path: one workgroup of NT wavefronts per (chain, segment).  At d = 49…64 the forward kernel keeps two
// matrices in LDS and 254 registers, so TWO workgroups share a CU (one wavefront of each per SIMD): measured at C3,
// forward 0.72 -> 0.58 ms with 500 instead of 250 segments (750: 0.62).  The smaller tiles leave room for more, and the
// kernels are latency-bound, so
// more resident workgroups pay until the per-segment prologue dominates (measured, scripts/time_mid_dims.py:
// d = 16, 512 chains, T = 1000: 4.27 ms with 2 workgroups per CU, 2.22 ms with 48; d = 32, 128 chains: 4.86 -> 3.02 ms).
// d ≥ 48: two workgroups fit a CU; a time-invariant chain gets four workgroups' worth of segments, because most of them leave the sweep kernels
// after two or three steps (their matrices repeat: kd_forward_info FROZEN) and the sweep is as long as the segments that do not — measured at C3
// (scripts/time_c3_clean.py, C3_SEGMENTS): 0.578 ms with 715 segments, 0.553 with 909, 0.547 – 0.557 with 1000, 0.559 with 1111, 0.605 with 1429
// (with three repeats required before a segment leaves: 0.670 with 500, 0.612 with 715, 0.626 with 1000)
inline Segmentation segmentation(const Shape& s, const Flags& f, const ScheduleHooks& hooks) {
    Segmentation g;
    const bool dense = s.dense;
    const bool dense_frozen = dense && f.nt >= 3 && f.uniform && !f.masked && !s.step_model && !f.gseq;
    const int dense_wg_per_cu = !dense ? 0 : f.nt == 1 ? 48 : f.nt == 2 ? 8 : dense_frozen ? 4 : 2;
    const long long steps = s.T - 1;  // transitions
    if (steps <= 0) {
        g.S = 0;
        g.L = 1;
        g.Llast = 1;
        return g;
    }
    long long S_target = (f.sequential && hooks.one_segment) ? 1 : s.segments > 0 ? s.segments
                         : dense ? (256 * dense_wg_per_cu + f.wg_chains - 1) / f.wg_chains
                                 : (131072 + s.n_chains - 1) / s.n_chains;
    if (s.segments <= 0 && !dense) {
        // few chains: the lanes do not fill the machine and the sweep is a latency chain of L steps through three
        // kernels (≈0.86 µs per step, fitted at d = 2) plus S sequential boundary steps (≈0.26 µs each):
        // S* = sqrt(steps · 0.86 / 0.26).  (measured, one chain, d = 2, T = 50 000: 1.18 ms with L = 16, S = 3125.)
        const long long s_lat = (long long)std::ceil(std::sqrt(3.3 * (double)steps));
        if (S_target > s_lat) S_target = s_lat;
        // a few chains whose lanes fit ONE workgroup run the whole sweep in one launch (k_small_sweep: chains · S ≤ 256, ≤ 64 chains):
        // take fewer, slightly longer segments for that where it costs at most a few steps of latency
        const long long cap = s.n_chains <= 16 ? 256 / s.n_chains : 0;
        if (cap >= 1 && S_target > cap && (steps + cap - 1) / cap <= 32) S_target = cap;
        // … and with its boundary recursion in log depth (boundary_scan_par_body) the segments of that schedule can be SHORT: as many as
        // fit the workgroup, down to 3 steps each (measured, scripts/time_small_segments.py)
        if (cap >= 1 && (steps + cap - 1) / cap <= 32 && f.uniform && !f.masked && !s.step_model && !hooks.small_sweep_off) {
            S_target = std::min<long long>(cap, std::max<long long>(1, steps / 3));
            g.small_short = true;
        }
    }
    // Batches of one model on the model / data split (split_wanted): the data pass is vectors only, one workgroup per 4·(64/d) chains
    // of a segment, so the machine fills through MORE segments, and the per-model tables are a recursion over the segment LENGTH
    // (kt_gains, kt_agg: sequential in L).  Segments of ≈32 steps, at most 128 of them (measured, scripts/time_split_segments.py:
    // d = 64 × 64 chains × T = 1000: sweep 1.60 -> 1.21 ms and first touch 23 -> 8.5 ms with 32 instead of 8 segments; d = 32 × 256:
    // 1.25 -> 1.09 ms, 10.6 -> 4.5 ms; d = 8 × 1024: 0.48 -> 0.46 ms).
    const bool split_eligible = dense && !f.gseq && s.n_models == 1 && split_wanted(f.wg_chains, hooks);
    if (split_eligible && s.segments <= 0) S_target = std::max(S_target, std::min<long long>(128, (steps + 31) / 32));
    if (S_target < 1) S_target = 1;
    long long L = (steps + S_target - 1) / S_target;
    const long long Lmin = s.segments > 0 ? 1 : g.small_short ? 3 : 8;
    if (L < Lmin) L = Lmin;
    if (L > steps) L = steps;
    g.L = L;
    g.S = (int)((steps + L - 1) / L);
    g.Llast = steps - (long long)(g.S - 1) * L;
    return g;
}

// The one-pass schedule (k_forward0 + table-driven backward sweep) pays where the sweep is bandwidth-bound.  A few chains
// are a latency chain of L steps either way, and its tables cost 30 µs more at creation (measured, one chain, T = 10⁴:
// 0.41 against 0.38 ms end to end), so small problems keep the two-pass schedule.  RXHIP_ONE_PASS=0/1 overrides (tests).
inline bool want_fused(bool uniform, int S, long long n_chains, long long T, const ScheduleHooks& hooks) {
    return uniform && S > 0 && (hooks.one_pass >= 0 ? hooks.one_pass != 0 : (double)n_chains * (double)T >= 4194304.0);
}
// the tables of the table-driven backward sweep (k_backward_sh) exist: batches of a multiple of 64 chains
inline bool gtab_tables(long long n_chains, const ScheduleHooks& hooks) { return n_chains % 64 == 0 && !hooks.backward_lanes; }
// Reverse-filter candidates (k_backward_sh_rev): the table-driven backward sweep, no more observation than
// state components (the observations it reads instead of the z records are not larger).  The stride is chosen once
// the tables exist; RXHIP_MEAN_RECORDS=1 keeps a record per time index, RXHIP_MEAN_CHECKPOINT=K forces the stride K.
inline bool rev_cand(bool fused, long long n_chains, int d, int dy, long long T, const ScheduleHooks& hooks) {
    return fused && gtab_tables(n_chains, hooks) && dy <= d && T > 1 && !hooks.mean_records;
}

// Wavefronts per workgroup of the two sweep kernels of the reverse-filter schedule (k_forward0_ck, k_backward_sh_rev): the W waves of a
// workgroup take W adjacent 64-chain groups of one segment and share one table stream, so 64·W must divide the batch.  Each kernel ships the
// width that won its own arm comparison in every round (profiles/r14/README.md): the backward sweep two waves (0.01–0.03 ms ahead of one; four
// are no better than two), the forward kernel one (no width was ahead in every round).  RXHIP_SWEEP_WAVES forces one width for both (0: not
// forced; the caller has refused a forced width that does not divide the batch).
constexpr int SWEEP_WAVES_FORWARD = 1, SWEEP_WAVES_BACKWARD = 2;
inline bool sweep_waves_divide(long long n_chains, int w) { return w >= 1 && n_chains % (64LL * w) == 0; }
inline int sweep_waves(long long n_chains, int shipped, int forced) {
    if (forced > 0) return forced;
    for (int w = 4; w > 1; w >>= 1)
        if (w <= shipped && sweep_waves_divide(n_chains, w)) return w;
    return 1;
}

}  // namespace plan
}  // namespace rxhip
