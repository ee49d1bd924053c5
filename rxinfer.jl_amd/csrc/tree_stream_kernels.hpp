// tree_stream_kernels.hpp — the per-observation step of rxhip_tree_stream (include/rxhip.h "Streaming"): what the loop of src/inference/streaming.jl:341-407 does
// between two observations, on the device.  ONE kernel, launched twice per observation over a table of rows (a row: one double of one replica's state):
//   before the iterations   feedback rows (a target's value slot ← the source's marginal: its mean, its variance, or 1 / variance — the @autoupdates fetched once
//                           per observation, src/inference/autoupdates.jl) and series rows (a data variable's value slot ← observation t of the uploaded series);
//   behind them             history rows (mean | packed covariance of a history variable's marginal → the observation's block of the device-resident history).
// The sweeps in between are the executor's own launches (tree_engine.hip): nothing here touches a message, and no existing kernel knows about streams.
// Layouts (TreeParams in tree_kernels.hpp): element k of replica r of an array lives at k·es + r·rs — replica-fastest (es = RS, rs = 1) for the lane kernels, a
// replica's slots contiguous (es = 1, rs = slots per replica) for the wavefront / workgroup kernels.  The series and the history are stored the same way
// (transposed once at upload / once at read-back), so every load and store of a wavefront runs along the stride-1 index: consecutive lanes take consecutive
// replicas of one row, or consecutive rows of one replica.  Only replicas r < R are touched: the padding between R and RS keeps the zeros it was allocated with.
#pragma once
#include <hip/hip_runtime.h>

namespace rxhip {
namespace tree {

enum StreamRowKind { SR_SERIES = 0, SR_MEAN = 1, SR_VAR = 2, SR_PRECISION = 3, SR_HISTORY = 4 };
struct StreamRow {
    int dst;    // value slot (SERIES, feedback) or history row (HISTORY)
    int src;    // series column (SERIES) or marginal slot (feedback, HISTORY)
    int kind;   // StreamRowKind
    int init;   // feedback: index into StreamStep.init — the source's `@initialization` marginal, read instead of the marginal before a fresh engine's first observation
};
struct StreamStep {
    const StreamRow* rows;
    int n_rows;
    int by_replica;   // 1: a replica's slots are contiguous (es = 1) — items run rows-fastest; 0: replica-fastest
    long long R;
    double* val;         long long es_val, rs_val;
    const double* marg;  long long es_marg, rs_marg;
    const double* series; long long es_ser, rs_ser;   // observation t: column k of replica r at series[k·es_ser + r·rs_ser]
    double* hist;        long long es_hist, rs_hist;  // observation t: row q of replica r at hist[q·es_hist + r·rs_hist]
    const double* init;  // nullptr: the feedback reads the current marginals
};

__global__ void __launch_bounds__(256) k_tree_stream_step(const StreamStep c) {
    const long long n = c.n_rows, total = n * c.R;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long q = c.by_replica ? i % n : i / c.R, r = c.by_replica ? i / n : i % c.R;
        const StreamRow w = c.rows[q];
        if (w.kind == SR_SERIES)
            c.val[(long long)w.dst * c.es_val + r * c.rs_val] = c.series[(long long)w.src * c.es_ser + r * c.rs_ser];
        else if (w.kind == SR_HISTORY)
            c.hist[(long long)w.dst * c.es_hist + r * c.rs_hist] = c.marg[(long long)w.src * c.es_marg + r * c.rs_marg];
        else {
            const double x = c.init ? c.init[w.init] : c.marg[(long long)w.src * c.es_marg + r * c.rs_marg];
            c.val[(long long)w.dst * c.es_val + r * c.rs_val] = w.kind == SR_PRECISION ? 1.0 / x : x;   // (MEAN / VAR: a copy — the bits the host loop would send back)
        }
    }
}

}  // namespace tree
}  // namespace rxhip
