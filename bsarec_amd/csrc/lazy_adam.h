// Lazy (sparse) Adam for the item table under the sampled-softmax head (bsarec_config_t.train_lazy_adam, include/bsarec_hip.h).
// A step updates only the item rows it touches -- T = the looked-up ids != 0, the answers and the N candidates -- so the
// item table's share of the optimiser costs O(|T| d) instead of O(V d).  The pieces, all on the device (a captured step
// replays with a fresh T):
//   LazyRows       a per-plan int32[V] mark array (0 between steps) and a compact list of the marked rows with its count.
//                  The count is reset by ssm_logits_kernel (the step's loss, before anything marks); ssm_bwd_kernel marks
//                  (lazy_mark_wave: the first marker of a row appends it, one atomic per wave); the step's last item-table
//                  pass clears the marks of the listed rows again.
//   lookup flush   (kernels.h, LookupAcc.lazy) the fixed-point accumulator -> the gradient rows of T, not the V rows
//   lazy Adam      reduce_adam_kernel's item arm (fused indexed step, kernels.h) or lazy_adam_kernel here (every other step
//                  shape): the arithmetic of adam_kernel on the rows of T only (lazy_adam_rows, lazy_adam4)
// Rows are listed in arbitrary order; each row's update is independent of the others, so the step stays bit-deterministic.
// The restatement in numpy is tests/lazy_adam_ref.py.
#pragma once
#include "common.h"

struct LazyRows {
    int* mark;           // [V]: 1 while the row is in this step's list, else 0
    int* rows;           // [cap]: the touched rows of the step, in arbitrary order
    int* count;          // rows listed so far (reset once per step)
    int cap;             // min(V, B L + B + N): no step can touch more distinct rows
    int d4;              // float4 groups per row (d / 4)
};

// Mark row r (valid lanes only); the first marker of the step appends it to the list.  Called by all 64 lanes of a wave
// together (the ballot): one global atomic per wave for the slots (Guideline 12: wave-aggregated atomics).
__device__ __forceinline__ void lazy_mark_wave(const LazyRows& T, int r, bool valid) {
    const bool first = valid && atomicExch(T.mark + r, 1) == 0;
    const unsigned long long won = __ballot(first);
    if (won == 0ull) return;                                      // wave-uniform
    const int lane = threadIdx.x & 63, leader = __builtin_ctzll(won);
    int base = 0;
    if (lane == leader) base = atomicAdd(T.count, __popcll(won));
    base = __shfl(base, leader);
    if (first) {
        const int slot = base + __popcll(won & ((1ull << lane) - 1ull));
        if (slot < T.cap) T.rows[slot] = r;                       // (never false: at most cap distinct rows are marked)
    }
}

// The marking role over ids [nids] (0 = padding, not marked), answers [B] and cand [N], clamped to [0, V): element e of the
// concatenation, grid-stride from wave-aligned starts so that every lane of a wave takes the same trips.  Only ids of the
// owned window [lo, lo + Vs) are marked, at their local index (the plan owns [0, V)).
template <class I>
__device__ __forceinline__ void lazy_mark_role(const LazyRows& T, const I* __restrict__ ids, long nids,
                                               const int64_t* __restrict__ answers, int B, const int* __restrict__ cand, int N,
                                               long V, long lo, long Vs, int blk, int nblk) {
    const long total = nids + B + N, stride = (long)nblk * ROW_THREADS;
    for (long e0 = (long)blk * ROW_THREADS + (threadIdx.x & ~63); e0 < total; e0 += stride) {
        const long e = e0 + (threadIdx.x & 63);
        long id = 0;
        bool valid = e < total;
        if (valid) {
            id = e < nids ? (long)ids[e] : (e < nids + B ? (long)answers[e - nids] : (long)cand[e - nids - B]);
            id = id < 0 ? 0 : (id >= V ? V - 1 : id);
            valid = (e >= nids || id != 0) && id >= lo && id < lo + Vs;
        }
        lazy_mark_wave(T, valid ? (int)(id - lo) : 0, valid);
    }
}

// The rows of T, grid-stride from `first`: fn(r, q, i) for float4 group q of listed row r, i = r d4 + q its group index
template <class F>
__device__ __forceinline__ void lazy_rows_walk(const LazyRows& T, long first, long stride, F fn) {
    const int d4 = T.d4;
    const long n = (long)min(*T.count, T.cap) * d4;
    for (long k = first; k < n; k += stride) {
        const int r = T.rows[k / d4], q = (int)(k % d4);
        fn(r, q, (long)r * d4 + q);
    }
}

// One float4 group of Adam, the arithmetic of adam_kernel / reduce_adam_kernel's item arm expression for expression.
__device__ __forceinline__ void lazy_adam4(f32x4& wi, f32x4& mi, f32x4& vi, f32x4 gi, float b1, float b2, float eps, float wd,
                                           float step_size, float bc2s) {
    if (wd != 0.f) gi += wd * wi;
    mi = b1 * mi + (1.0f - b1) * gi;
    vi = b2 * vi + (1.0f - b2) * gi * gi;
#pragma unroll
    for (int k = 0; k < 4; ++k) wi[k] -= step_size * (mi[k] / (sqrtf(vi[k]) / bc2s + eps));
}

// Adam of the float4 group at element offset o of w / m / v with gradient gi
__device__ __forceinline__ void lazy_adam_at(float* w, float* m, float* v, long o, f32x4 gi, float b1, float b2, float eps, float wd,
                                             float step_size, float bc2s) {
    f32x4 wi = ld4(w + o), mi = ld4(m + o), vi = ld4(v + o);
    lazy_adam4(wi, mi, vi, gi, b1, b2, eps, wd, step_size, bc2s);
    st4(w + o, wi); st4(m + o, mi); st4(v + o, vi);
}

// The step's last pass over T: Adam of every listed row of the item table at element offset off of w / m / v, then the row's
// mark cleared.  grad(i, o) returns the gradient of group i (element offset o = off + 4 i) and leaves the gradient row as
// the caller wants it after the step.
template <class FG>
__device__ __forceinline__ void lazy_adam_rows(const LazyRows& T, long first, long stride, float* w, float* m, float* v, long off,
                                               float b1, float b2, float eps, float wd, float step_size, float bc2s, FG grad) {
    lazy_rows_walk(T, first, stride, [&](int r, int q, long i) {
        const long o = off + 4 * i;
        lazy_adam_at(w, m, v, o, grad(i, o), b1, b2, eps, wd, step_size, bc2s);
        if (q == 0) T.mark[r] = 0;
    });
}

// The plan-aware Adam of a lazy step whose update is not fused into the gradient reduction: blocks [0, dense_blocks) run
// adam_kernel's update over the arena without the item table ([0, item_off) and [item_off + item_n, n)), the others the
// rows of T (their gradient rows were written by the lookup flush).  t / bias corrections: already advanced (state[3]).
struct LazyAdamP {
    float *w; const float* g; float *m, *v;
    long n, item_off, item_n;            // arena length, the item table's element offset and length (all % 4 == 0)
    float b1, b2, eps, wd, gscale;
    int dense_blocks;
    LazyRows T;
};
__global__ void __launch_bounds__(ROW_THREADS)
lazy_adam_kernel(const uint64_t* __restrict__ state, const LazyAdamP A) {
    const float* f = reinterpret_cast<const float*>(state + 3);
    const float step_size = f[0], bc2s = f[1];
    if ((int)blockIdx.x < A.dense_blocks) {
        const long lo4 = A.item_off / 4, skip4 = A.item_n / 4, n4 = (A.n - A.item_n) / 4;
        for (long j = (long)blockIdx.x * ROW_THREADS + threadIdx.x; j < n4; j += (long)A.dense_blocks * ROW_THREADS) {
            const long o = 4 * (j < lo4 ? j : j + skip4);
            lazy_adam_at(A.w, A.m, A.v, o, ld4(A.g + o) * A.gscale, A.b1, A.b2, A.eps, A.wd, step_size, bc2s);
        }
        return;
    }
    const long nb = gridDim.x - A.dense_blocks;
    lazy_adam_rows(A.T, (long)(blockIdx.x - A.dense_blocks) * ROW_THREADS + threadIdx.x, nb * ROW_THREADS, A.w, A.m, A.v, A.item_off,
                   A.b1, A.b2, A.eps, A.wd, step_size, bc2s, [&](long, long o) { return ld4(A.g + o) * A.gscale; });
}

// Lazy Adam of a catalogue shard (include/bsarec_shard.h, bsarec_shard_lazy_adam): the rows of T (marked by
// shard_lazy_mark_kernel, catalogue_shard.h) of the shard's w / m / v with its gradient g and the corrections of the step's
// tick (state[3]); the gradient rows are zeroed.  Rows outside T are not read.
struct ShardLazyAdamP { float *w, *g, *m, *v; float b1, b2, eps, wd; LazyRows T; };
__global__ void __launch_bounds__(ROW_THREADS)
shard_lazy_adam_kernel(const uint64_t* __restrict__ state, const ShardLazyAdamP A) {
    const float* f = reinterpret_cast<const float*>(state + 3);
    lazy_adam_rows(A.T, (long)blockIdx.x * ROW_THREADS + threadIdx.x, (long)gridDim.x * ROW_THREADS, A.w, A.m, A.v, 0, A.b1, A.b2,
                   A.eps, A.wd, f[0], f[1], [&](long, long o) {
                       const f32x4 gi = ld4(A.g + o);
                       st4(A.g + o, f32x4{0.f, 0.f, 0.f, 0.f});
                       return gi;
                   });
}
