// Full-catalogue cross-entropy on an external hidden state (bsarec_ce_head_fwd / bsarec_ce_head_bwd, include/bsarec_hip.h):
// loss = mean_b (lse_b - s(b, a_b)), d(h) and dE, without anything of size B x V.  Every kernel forms its scores again, 32 x 32
// at a time, through score_tile (score_tile.h: the fmaf chain of fr_dot bit for bit), so the backward's softmax is built from
// the bits the forward's row statistics were built from.
//
// Launch shape.  A workgroup is 4 waves; a wave owns 32 items of a 128-item block and RB row blocks of 32 rows whose h rows sit in
// LDS (score_stage).  Whichever way round score_tile takes its operands (ROWS_IN_LANE: a lane holds one row and 16 items; else
// one item and 16 rows), register r of the result is the A operand of k-step r of a second MFMA whose k axis is the axis the lane
// holds 16 of, with no exchange through LDS: k-step r takes k = rho(r) from lanes 0..31 and k = rho(r) + 4 from lanes 32..63.
//   forward:  ce_fwd_kernel   grid (S, ceil(B / 128)), ROWS_IN_LANE: a split owns a contiguous range of item blocks; per lane and
//                             row block ONE online (max, sum), updated per block of 16 scores; merged over the two halves, then
//                             over the waves in wave order -> (m, l)[split][row]
//             ce_stat_kernel  one workgroup: merges the S partials of a row in split order -> m, log l; s(b, a_b) by fr_dot;
//                             rows_out; the mean in a fixed order (mean_of_1024) -> loss_out
//   backward: ce_dh_kernel    grid (S, ceil(B / (32 RB))), ROWS_IN_LANE: G = exp((s - m) - log l) - [j == a]; acc[rows x d] += G . E with
//                             E's rows as the B operand (32 consecutive floats per half-wave); the four waves' tiles are added
//                             in wave order through LDS and stored to the split's slab.  RB x ceil(d / 32) <= 8 register tiles.
//             ce_dh_sum_kernel  dh = g / B * (the slabs added in split order)
//             ce_de_kernel    one workgroup per item block, !ROWS_IN_LANE: loops over ALL row tiles of 128, acc[items x d] +=
//                             G^T . h with h's LDS rows as the B operand; dE row j = g / B * acc -- one writer per row, one order
// No atomics, no host synchronisation, no allocation: capturable and bit-deterministic; h is read through its row stride only.
// S: min(item blocks, ceil(1024 / row tiles), max(1, 16384 / B)), so S B <= 16384 + B whatever V is.
// The row statistics stay in two parts, the maximum m and log l: lse = m + log l rounds at the magnitude of m (half an ulp of 100
// is 3.8e-6, relative, in every exp(s - lse) of the row), (s - m) - log l does not; row = (m - s_a) + log l likewise.
// Workspace (floats): m[B] | logl[B] | pm[S][B] | pl[S][B] | pad to 4 | slab[S][B][d].
//
// Range form (bsarec_ce_head_range_stats / _merge / _bwd): E holds rows [base, base + V) of a catalogue of N rows, one shard of a
// table split by rows.  Items, tiles and every comparison j == a stay LOCAL; the base enters in ce_answer alone, which clamps the
// answer to [0, N) globally and gives its local index, or CE_NO_ANSWER when another range owns it.  The single-table entry
// points are base 0, N = V of the same kernels.  Between the forward and the backward the ranges exchange a row's (max, sum,
// target score): ce_stat_kernel<true> writes them, ce_merge_kernel merges every range's in range order and leaves the whole
// catalogue's m and log l in the workspace slots the backward kernels read.
#pragma once
#include "full_rank.h"

#define CE_ITEMS 128                       // items per block: 4 waves x 32
#define CE_ROWS 128                        // rows per tile of the forward and of the dE kernel

struct CeP {
    const float* h; long ldh;
    const float* E;
    const int64_t* ans;
    int B, V, d, S, nblk;                    // V: the rows of E
    int N; long base;                        // E's rows are items [base, base + V) of N
    float *m, *logl, *pm, *pl, *slab;        // the workspace
    const int32_t* rows;                     // row r is row rows[r] of h and of dh; null: the identity
    const int32_t* count;                    // device scalar: the first min(count[0], B) rows are live; null: all B
};
// Row list and live count (the cloze head, cloze.h's output): B stays the CAPACITY -- it sizes the splits, the workspace and the
// grids on the host -- and n = ce_live(P) <= B rows exist.  A row tile at or behind n exits at once, the dE kernel's row loop
// ends at n, every mean is over max(n, 1), and an entry of the list at or behind n is never read as an index.  The plain and
// range entry points pass (null, null): n = B and row r = r, the bits they always gave.
__device__ __forceinline__ int ce_live(const CeP& P) {
    if (!P.count) return P.B;
    const int n = *P.count;
    return n < 0 ? 0 : (n < P.B ? n : P.B);
}
__device__ __forceinline__ long ce_row(const CeP& P, int r) { return P.rows ? (long)P.rows[r] : (long)r; }
__device__ __forceinline__ float ce_mean_div(int n) { return (float)(n > 0 ? n : 1); }

static inline int ce_nblk(int V) { return (int)(((long)V + CE_ITEMS - 1) / CE_ITEMS); }
static inline int ce_splits(int B, int V) {
    const int T = (B + CE_ROWS - 1) / CE_ROWS;
    int S = (1024 + T - 1) / T;
    const int cap = 16384 / B > 1 ? 16384 / B : 1;
    if (S > cap) S = cap;
    const int nblk = ce_nblk(V);
    return S > nblk ? nblk : S;
}
static inline long ce_stat_floats(long B, long S) { return (2 * B + 2 * S * B + 3) / 4 * 4; }
static inline long ce_workspace_floats(int B, int V, int d) {
    const long S = ce_splits(B, V);
    return ce_stat_floats(B, S) + S * B * d;
}
// row blocks of the dh kernel for NDC = 1, 2, 4, 8 column blocks of 32: RB x NDC x 16 accumulator registers (<2, 8> spills)
static inline int ce_dh_rb(int ndc) { return ndc <= 2 ? 4 : (ndc <= 4 ? 2 : 1); }
static inline int ce_ndc(int d) { const int n = (d + 31) / 32; return n <= 2 ? n : (n <= 4 ? 4 : 8); }

#define CE_NO_ANSWER 0xffffffffu             // of a tile row behind B, of an answer in another range: no item index reaches it
                                             // (V + 127 < 2^32)
// the local index of row b's answer (clamped to [0, N) globally), or CE_NO_ANSWER when it lies outside [base, base + V)
__device__ __forceinline__ unsigned ce_answer(const CeP& P, int b) {
    const long a = P.ans[b];
    const long c = (a < 0 ? 0 : (a >= P.N ? P.N - 1 : a)) - P.base;
    return c >= 0 && c < P.V ? (unsigned)c : CE_NO_ANSWER;
}

// grid (S, row tiles).  Dynamic LDS: CE_ROWS x (d + 4) floats of h.
__global__ void __launch_bounds__(ROW_THREADS) ce_fwd_kernel(const CeP P) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    __shared__ float wm[ROW_THREADS / 64][CE_ROWS], wl[ROW_THREADS / 64][CE_ROWS];
    constexpr int RB = CE_ROWS / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, half = lane >> 5;
    const int r0 = blockIdx.y * CE_ROWS, n = ce_live(P);
    if (r0 >= n) return;
    int b0, b1;
    split_range(blockIdx.x, P.nblk, P.S, b0, b1);           // this split's item blocks
    score_stage(P.h, P.ldh, n, P.d, r0, CE_ROWS, sh, P.rows);
    __syncthreads();
    float m[RB], l[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) { m[rb] = -INFINITY; l[rb] = 0.f; }
    for (int ib = b0; ib < b1; ++ib) {
        const unsigned i0 = (unsigned)ib * CE_ITEMS + wave * 32;         // this wave's 32 items
        unsigned eoff;
        const float* eb = score_items(P.E, P.V, P.d, i0, eoff);
        f32x16 acc[RB];
        score_tile<RB, true>(sh, eb, eoff, P.d, acc);
        const bool tail = i0 + 32 > (unsigned)P.V;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (tail && i0 + rho(r) + 4 * half >= (unsigned)P.V) acc[rb][r] = -INFINITY;
                mx = fmaxf(mx, acc[rb][r]);
            }
            const float M = fmaxf(m[rb], mx);
            if (M == -INFINITY) continue;
            float add = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) add += expf(acc[rb][r] - M);
            l[rb] = l[rb] * expf(m[rb] - M) + add;
            m[rb] = M;
        }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const float m2 = __shfl_xor(m[rb], 32, 64), l2 = __shfl_xor(l[rb], 32, 64);
        float ma = half ? m2 : m[rb], la = half ? l2 : l[rb];            // both halves merge (half 0, half 1) in that order
        softmax_merge(ma, la, half ? m[rb] : m2, half ? l[rb] : l2);
        if (half == 0) { wm[wave][rb * 32 + l31] = ma; wl[wave][rb * 32 + l31] = la; }
    }
    __syncthreads();
    if (tid < CE_ROWS && r0 + tid < n) {
        float mm = wm[0][tid], ll = wl[0][tid];
#pragma unroll
        for (int w = 1; w < ROW_THREADS / 64; ++w) softmax_merge(mm, ll, wm[w][tid], wl[w][tid]);
        P.pm[(long)blockIdx.x * P.B + r0 + tid] = mm;
        P.pl[(long)blockIdx.x * P.B + r0 + tid] = ll;
    }
}

// one workgroup of 1024 lanes.  !RANGE: m, log l, rows_out, loss.  RANGE: rows_out is stats[3][B] -- the range's maximum, its
// sum and the answer's score where the range owns the answer, else 0 (S = 0, a range without rows: -inf, 0, 0); no loss.
template <bool RANGE>
__global__ void __launch_bounds__(1024) ce_stat_kernel(const CeP P, float* __restrict__ loss_out, float* __restrict__ rows_out) {
    const int tid = threadIdx.x, n = ce_live(P);
    float sum = 0.f;
    if (!RANGE && rows_out)
        for (int b = n + tid; b < P.B; b += 1024) rows_out[b] = 0.f;
    for (int b = tid; b < n; b += 1024) {
        const SoftmaxPart part = softmax_merge_splits(P, P.B, b);
        const float m = part.m, l = part.l;
        if (RANGE) {
            const unsigned a = ce_answer(P, b);
            rows_out[b] = m;
            rows_out[P.B + b] = l;
            rows_out[2 * P.B + b] = a == CE_NO_ANSWER ? 0.f : fr_dot(P.h + ce_row(P, b) * P.ldh, P.E + (long)a * P.d, P.d);
            continue;
        }
        const float logl = logf(l);
        const float row = (m - fr_dot(P.h + ce_row(P, b) * P.ldh, P.E + (long)ce_answer(P, b) * P.d, P.d)) + logl;
        P.m[b] = m;
        P.logl[b] = logl;
        if (rows_out) rows_out[b] = row;
        sum += row;
    }
    if (!RANGE) mean_of_1024(sum, n > 0 ? n : 1, loss_out);
}

// one workgroup of 1024 lanes: stats_all[world][3][B], every range's ce_stat_kernel<true> output in range order -> the whole
// catalogue's m and log l (the slots of ce_dh_kernel / ce_de_kernel), loss_rows, loss.  A range without rows, (-inf, 0), is
// neutral in softmax_merge: M is the other maximum, and l * expf(0) + 0 * expf(-inf) = l exactly.  One range: what
// ce_stat_kernel<false> writes, bit for bit.  The target is the sum over the ranges: one owner, the others wrote 0.
__global__ void __launch_bounds__(1024) ce_merge_kernel(const float* __restrict__ stats_all, int world, int B, float* __restrict__ m_out,
                                                        float* __restrict__ logl_out, float* __restrict__ loss_rows,
                                                        float* __restrict__ loss_out) {
    const int tid = threadIdx.x;
    float sum = 0.f;
    for (int b = tid; b < B; b += 1024) {
        float m = -INFINITY, l = 0.f, target = 0.f;
        for (int w = 0; w < world; ++w) {
            const float* s = stats_all + (long)w * 3 * B;
            softmax_merge(m, l, s[b], s[B + b]);
            target += s[2 * B + b];
        }
        const float logl = logf(l);
        const float row = (m - target) + logl;
        m_out[b] = m;
        logl_out[b] = logl;
        loss_rows[b] = row;
        sum += row;
    }
    mean_of_1024(sum, B, loss_out);
}

// grid (S, ceil(B / (32 RB))).  Dynamic LDS: 32 RB x (d + 4) floats: the h tile, then the waves' sum.
template <int RB, int NDC>
__global__ void __launch_bounds__(ROW_THREADS) ce_dh_kernel(const CeP P) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    constexpr int ROWS = 32 * RB;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, half = lane >> 5;
    const int r0 = blockIdx.y * ROWS, dp = P.d + 4, n = ce_live(P);
    if (r0 >= n) return;
    int b0, b1;
    split_range(blockIdx.x, P.nblk, P.S, b0, b1);           // this split's item blocks
    score_stage(P.h, P.ldh, n, P.d, r0, ROWS, sh, P.rows);
    float mx[RB], logl[RB];
    unsigned ans[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int b = r0 + rb * 32 + l31;
        mx[rb] = b < n ? P.m[b] : 0.f;
        logl[rb] = b < n ? P.logl[b] : 0.f;
        ans[rb] = b < n ? ce_answer(P, b) : CE_NO_ANSWER;
    }
    __syncthreads();
    f32x16 out[RB][NDC];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int dc = 0; dc < NDC; ++dc)
#pragma unroll
            for (int r = 0; r < 16; ++r) out[rb][dc][r] = 0.f;
    for (int ib = b0; ib < b1; ++ib) {
        const unsigned i0 = (unsigned)ib * CE_ITEMS + wave * 32;
        unsigned eoff;
        const float* eb = score_items(P.E, P.V, P.d, i0, eoff);
        f32x16 acc[RB];
        score_tile<RB, true>(sh, eb, eoff, P.d, acc);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned j = i0 + rho(r) + 4 * half;
                const float g = expf((acc[rb][r] - mx[rb]) - logl[rb]) - (j == ans[rb] ? 1.f : 0.f);
                acc[rb][r] = j < (unsigned)P.V ? g : 0.f;
            }
#pragma unroll
        for (int dc = 0; dc < NDC; ++dc) {
            const int c = dc * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {                               // k-step r: item rho(r) from lanes 0..31, + 4 from 32..63
                const bool on = i0 + rho(r) + 4 * half < (unsigned)P.V && c < P.d;
                const float ev = on ? eb[(unsigned)((rho(r) + 4 * half) * P.d + c)] : 0.f;
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) out[rb][dc] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[rb][r], ev, out[rb][dc], 0, 0, 0);
            }
        }
    }
    // out[rb][dc][r] is row 32 rb + rho(r) + 4 half, column 32 dc + l31: the four waves add up in wave order
    for (int w = 0; w < ROW_THREADS / 64; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int dc = 0; dc < NDC; ++dc)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int c = dc * 32 + l31;
                        if (c < P.d) {
                            float* p = &sh[(rb * 32 + rho(r) + 4 * half) * dp + c];
                            *p = w == 0 ? out[rb][dc][r] : *p + out[rb][dc][r];
                        }
                    }
        }
    }
    __syncthreads();
    float* slab = P.slab + (long)blockIdx.x * P.B * P.d;
    const int dq = P.d >> 2;
    for (int x = tid; x < ROWS * dq; x += ROW_THREADS) {
        const int i = x / dq, c = (x - i * dq) << 2;
        if (r0 + i < n) st4(slab + (long)(r0 + i) * P.d + c, ld4(&sh[i * dp + c]));
    }
}

// one lane per float4 of the live rows' gradient; row r goes to row ce_row(r) of dh (a row list: the caller zeroed dh)
__global__ void __launch_bounds__(ROW_THREADS) ce_dh_sum_kernel(const CeP P, const float* __restrict__ gout, float* __restrict__ dh) {
    const int n = ce_live(P);
    const long n4 = (long)n * P.d / 4, x = (long)blockIdx.x * ROW_THREADS + threadIdx.x;
    if (x >= n4) return;
    f32x4 v = ld4(P.slab + 4 * x);
    for (int s = 1; s < P.S; ++s) v += ld4(P.slab + (long)s * P.B * P.d + 4 * x);
    const unsigned e = (unsigned)(4 * x), r = e / (unsigned)P.d;                 // n d <= 2^24
    st4(dh + ce_row(P, (int)r) * P.d + (e - r * (unsigned)P.d), v * (*gout / ce_mean_div(n)));
}

// one workgroup per item block.  Dynamic LDS: CE_ROWS x (d + 4) floats of h.
template <int NDC>
__global__ void __launch_bounds__(ROW_THREADS) ce_de_kernel(const CeP P, const float* __restrict__ gout, float* __restrict__ dE) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    __shared__ float m_s[CE_ROWS], logl_s[CE_ROWS];
    __shared__ unsigned ans_s[CE_ROWS];
    constexpr int RB = CE_ROWS / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, half = lane >> 5;
    const int dp = P.d + 4, n = ce_live(P);
    const unsigned i0 = blockIdx.x * CE_ITEMS + wave * 32, mine = i0 + l31;
    unsigned eoff;
    const float* eb = score_items(P.E, P.V, P.d, i0, eoff);
    f32x16 out[NDC];
#pragma unroll
    for (int dc = 0; dc < NDC; ++dc)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[dc][r] = 0.f;
    for (int r0 = 0; r0 < n; r0 += CE_ROWS) {
        __syncthreads();
        score_stage(P.h, P.ldh, n, P.d, r0, CE_ROWS, sh, P.rows);
        if (tid < CE_ROWS) {
            m_s[tid] = r0 + tid < n ? P.m[r0 + tid] : 0.f;
            logl_s[tid] = r0 + tid < n ? P.logl[r0 + tid] : 0.f;
            ans_s[tid] = r0 + tid < n ? ce_answer(P, r0 + tid) : CE_NO_ANSWER;
        }
        __syncthreads();
        f32x16 acc[RB];
        score_tile<RB, false>(sh, eb, eoff, P.d, acc);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = rb * 32 + rho(r) + 4 * half;               // k-step (rb, r): row i of the tile; zero rows of h behind B
                const float g = expf((acc[rb][r] - m_s[i]) - logl_s[i]) - (mine == ans_s[i] ? 1.f : 0.f);
#pragma unroll
                for (int dc = 0; dc < NDC; ++dc) {
                    const int c = dc * 32 + l31;
                    const float hv = c < P.d ? sh[i * dp + c] : 0.f;
                    out[dc] = __builtin_amdgcn_mfma_f32_32x32x2f32(g, hv, out[dc], 0, 0, 0);
                }
            }
    }
    const float coef = *gout / ce_mean_div(n);
#pragma unroll
    for (int dc = 0; dc < NDC; ++dc)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned j = i0 + rho(r) + 4 * half;
            const int c = dc * 32 + l31;
            if (j < (unsigned)P.V && c < P.d) dE[(long)j * P.d + c] = out[dc][r] * coef;
        }
}
