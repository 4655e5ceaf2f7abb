// Sampled-softmax training head: every row b scores its answer a_b and N candidates n_0 .. n_N-1 shared by the batch, drawn
// with replacement from a Philox stream, with the logQ correction of popularity sampling.  Every product is a 64 x 64 output
// tile of one 256-thread workgroup (16-deep k-slices staged in LDS, 4 x 4 outputs per thread, fp32 FMAs -- the products are
// B N d, small next to the encoder; on gfx950 an fp32 MFMA would share the vector ALU anyway):
//   ssm_logits_kernel  (candidate tile, row tile): x_bj = h_b . E[n_j] - c(n_j), -inf on a hit
//   ssm_ce_kernel      (row): x_b0 = h_b . E[a_b] - c(a_b), logsumexp, loss_rows, dlogits = (softmax - onehot_0) inv_b
//   ssm_bwd_kernel     three roles in one grid: dE of the candidate columns (g^T H, summed over rows in a fixed order), the
//                      split-K slabs of dh = g . E_c that shard_slab_sum_kernel or the block backward sums, and dE of the
//                      answer columns (g_b0 h_b)
// The two callers differ in where an item row lives, where its gradient goes and who draws (template parameter GATHERED):
//   the plan (bsarec_config_t.train_negatives > 0, include/bsarec_hip.h; GATHERED = false): E is the item table [V][d], read
//     at the item's row; ssm_logits_kernel draws its tile's candidates itself from the plan's stream; dE is added as 64-bit
//     fixed point into the plan's item-table accumulator at the item's row.  Three launches per step.
//   the catalogue-sharded step (include/bsarec_shard.h, bsarec_shard_ssm_*; GATHERED = true): every rank draws the same N
//     candidates first (shard_ssm_draw_kernel), gathers their rows and its B answer rows out of the owners' shards
//     (shard_ssm_gather_kernel, catalogue_shard.h) into E = R [B + N][d] (answers first), read at the row's position, and runs
//     the head on its own B rows with inv_b = 1 / Bg; dE is this rank's dense partial G [B + N][d], overwritten (no fixed-point
//     accumulator: the owners sum the W partials, shard_ssm_pull_kernel).
// The restatement in numpy is tests/sampled_softmax_ref.py.
#pragma once
#include "kernels.h"
#include "sampled_rank.h"

#define SSM_NEG_MAX 8192                  // BSAREC_TRAIN_NEG_MAX
#define SSM_SITE 0x4E454753u              // BSAREC_TRAIN_NEG_SITE: Philox counter word 2 of the draws (no dropout site uses it)
#define SSM_TILE 64
#define SSM_KS 16                         // k-slice of the LDS-staged products
#define SSM_LDP 68                        // padded LDS row (floats): a 16-lane k-major store hits 16 distinct banks

struct SsmP {
    const float* H; long ldh;             // h_b = H[b * ldh .. + d)  (position L-1 of the last layer)
    const float* E;                       // item rows: the table [V][d], or the gathered rows R [B + N][d]
    const int64_t* answers;               // [B]
    const int64_t* pop_cum;               // popularity sampler: int64[V] cumulative counts; null: uniform over [1, V)
    const uint64_t* state;                // state[0] = key, state[1] = step (read on the device: graph replays draw afresh)
    int B, V, d, N, logq;                 // logq: subtract c(i) = log(N q_i) (popularity sampler, logQ on)
    float inv_b;
    int* cand; float* corr;               // [N] candidates, their corrections
    float* logits; float* dlogits;        // [B][N + 1], column 0 = the answer
    float* loss_rows;                     // [B]
    float* slab; int nslab, chunk;        // dh split-K slabs [nslab][B][d]; slab s sums candidate columns [s chunk, (s+1) chunk)
    unsigned long long* acc;              // plan: [V][d] fixed-point item-table accumulator (kernels.h, LookupAcc)
    float* G;                             // shard: [B + N][d] dense gradient of the gathered rows
    int tilesA, tilesB;                   // ssm_bwd_kernel: workgroups of the first two roles
    // lazy Adam step (lazy.rows != null, lazy_adam.h): ssm_logits_kernel resets the row count, and the last tilesM workgroups
    // of ssm_bwd_kernel mark the touched rows -- ids32 [nids] (!= 0), the answers and the candidates
    LazyRows lazy; const int* ids32; long nids; int tilesM;
};

// draw j of the step (0 <= j < N) -> item in [1, V) (uniform) or [0, V) with count > 0 (popularity)
__device__ __forceinline__ int ssm_draw(const SsmP& P, uint32_t k0, uint32_t k1, uint32_t step, int j) {
    if (!P.pop_cum) {
        const uint32_t call = (uint32_t)j >> 2;
        const uint4 w = philox4x32_10(call, 0u, SSM_SITE, step, k0, k1);
        const uint32_t m = j & 3, x = m == 0 ? w.x : (m == 1 ? w.y : (m == 2 ? w.z : w.w));
        return 1 + (int)(((uint64_t)x * (uint64_t)(P.V - 1)) >> 32);
    }
    const uint32_t call = (uint32_t)j >> 1;
    const uint4 w = philox4x32_10(call, 0u, SSM_SITE, step, k0, k1);
    const uint64_t x = (j & 1) ? ((uint64_t)w.z | ((uint64_t)w.w << 32)) : ((uint64_t)w.x | ((uint64_t)w.y << 32));
    const int64_t T = P.pop_cum[P.V - 1];
    const int it = neg_upper_bound(P.pop_cum, P.V, (int64_t)__umul64hi(x, (uint64_t)T));
    return it < P.V ? it : P.V - 1;
}

// c(i) = log(N q_i), q_i = count_i / T, in double then rounded once; 0 unless logq
__device__ __forceinline__ float ssm_corr(const SsmP& P, int i) {
    if (!P.logq || !P.pop_cum) return 0.f;
    const int64_t cnt = P.pop_cum[i] - (i > 0 ? P.pop_cum[i - 1] : 0);
    return (float)log((double)P.N * (double)cnt / (double)P.pop_cum[P.V - 1]);
}

// The row of E, and of its gradient, that holds candidate j (item it) / row b's answer: the item, or the gathered position
template <bool GATHERED> __device__ __forceinline__ long ssm_cand_row(const SsmP& P, int j, int it) { return GATHERED ? P.B + j : it; }
__device__ __forceinline__ int ssm_answer(const SsmP& P, int b) {
    const int a = (int)P.answers[b];
    return a < 0 ? 0 : (a >= P.V ? P.V - 1 : a);
}
template <bool GATHERED> __device__ __forceinline__ long ssm_answer_row(const SsmP& P, int b) { return GATHERED ? b : ssm_answer(P, b); }
// element k of that row's gradient: stored into G, or added to the accumulator (zeros skipped)
template <bool GATHERED> __device__ __forceinline__ void ssm_grad(const SsmP& P, long row, int k, float v) {
    if (GATHERED) P.G[row * P.d + k] = v;
    else if (v != 0.f) atomicAdd(P.acc + row * P.d + k, lookup_fix(v));
}

// acc[4][4] (rows r0 + i, columns c0 + j of a 64 x 64 tile) += sum_k A(k, r) B(k, c) over k in [0, K).  ldA(k, m) / ldB(k, m)
// return operand element (k, m) (0 out of range).  AK / BK: the operand is contiguous along k in memory -- then consecutive
// lanes take consecutive k of one m (coalesced), else consecutive m of one k.
template <bool AK, bool BK, class FA, class FB>
__device__ __forceinline__ void ssm_tile(int K, FA ldA, FB ldB, float (*As)[SSM_LDP], float (*Bs)[SSM_LDP], float acc[4][4]) {
    const int tid = threadIdx.x, r0 = (tid >> 4) * 4, c0 = (tid & 15) * 4;
    for (int k0 = 0; k0 < K; k0 += SSM_KS) {
        for (int i = tid; i < SSM_KS * SSM_TILE; i += ROW_THREADS) {
            const int ka = AK ? (i & 15) : (i >> 6), ma = AK ? (i >> 4) : (i & 63);
            const int kb = BK ? (i & 15) : (i >> 6), mb = BK ? (i >> 4) : (i & 63);
            As[ka][ma] = k0 + ka < K ? ldA(k0 + ka, ma) : 0.f;
            Bs[kb][mb] = k0 + kb < K ? ldB(k0 + kb, mb) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < SSM_KS; ++kk) {
            const f32x4 a = ld4(&As[kk][r0]), b = ld4(&Bs[kk][c0]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
}

// grid (ceil(N / 64), ceil(B / 64)): rows = batch rows, columns = candidates
template <bool GATHERED>
__global__ void __launch_bounds__(ROW_THREADS) ssm_logits_kernel(const SsmP P) {
    __shared__ __attribute__((aligned(16))) float As[SSM_KS][SSM_LDP];
    __shared__ __attribute__((aligned(16))) float Bs[SSM_KS][SSM_LDP];
    __shared__ int it_s[SSM_TILE];
    __shared__ float c_s[SSM_TILE];
    __shared__ long long ans_s[SSM_TILE];
    const int tid = threadIdx.x, col0 = blockIdx.x * SSM_TILE, row0 = blockIdx.y * SSM_TILE;
    // who draws resets the lazy row count, before anything marks
    if (!GATHERED && P.lazy.rows && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *P.lazy.count = 0;
    if (tid < SSM_TILE) {
        const int j = col0 + tid;
        int it = 0;
        float cj = 0.f;
        if (j < P.N) {
            if (GATHERED) { it = P.cand[j]; cj = P.corr[j]; }
            else {
                const uint64_t seed = P.state[0];
                it = ssm_draw(P, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)P.state[1], j);
                cj = ssm_corr(P, it);
                if (blockIdx.y == 0) { P.cand[j] = it; P.corr[j] = cj; }
            }
        }
        it_s[tid] = it; c_s[tid] = cj;
        const int b = row0 + tid;
        ans_s[tid] = b < P.B ? (long long)P.answers[b] : -1;
    }
    __syncthreads();
    float acc[4][4] = {};
    const int B = P.B, d = P.d;
    ssm_tile<true, true>(d,
        [&](int k, int m) { return row0 + m < B && k < d ? P.H[(long)(row0 + m) * P.ldh + k] : 0.f; },
        [&](int k, int m) { return col0 + m < P.N && k < d ? P.E[ssm_cand_row<GATHERED>(P, col0 + m, it_s[m]) * d + k] : 0.f; },
        As, Bs, acc);
    const int r0 = (tid >> 4) * 4, c0 = (tid & 15) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = row0 + r0 + i;
        if (b >= B) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            if (col0 + c >= P.N) continue;
            const float x = (long long)it_s[c] == ans_s[r0 + i] ? -INFINITY : acc[i][j] - c_s[c];
            P.logits[(long)b * (P.N + 1) + 1 + col0 + c] = x;
        }
    }
}

// The cross-entropy of one row over its n1 = N + 1 columns once the answer's logit is in row[0] (every lane has passed a
// barrier since): logsumexp, drow = (softmax - onehot_0) * inv_b, loss_row = lse - row[0].  One 256-lane workgroup; red /
// bc: the caller's LDS.
__device__ __forceinline__ void ssm_ce_row(const float* row, float* drow, int n1, float inv_b, float* loss_row, float* red,
                                           float& bc) {
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int j = tid; j < n1; j += ROW_THREADS) mx = fmaxf(mx, row[j]);
    mx = group_max<64>(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) { float m = red[0]; for (int i = 1; i < ROW_THREADS / 64; ++i) m = fmaxf(m, red[i]); bc = m; }
    __syncthreads();
    mx = bc;
    float s = 0.f;
    for (int j = tid; j < n1; j += ROW_THREADS) s += expf(row[j] - mx);      // exp(-inf) = 0: hits add nothing
    s = group_sum<64>(s);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) { float t = 0.f; for (int i = 0; i < ROW_THREADS / 64; ++i) t += red[i]; bc = mx + logf(t); }
    __syncthreads();
    const float lse = bc;
    for (int j = tid; j < n1; j += ROW_THREADS) drow[j] = (expf(row[j] - lse) - (j == 0 ? 1.0f : 0.0f)) * inv_b;
    if (tid == 0) *loss_row = lse - row[0];
}

// one workgroup per row: the answer's logit, then the row's cross-entropy over the N + 1 columns
template <bool GATHERED>
__global__ void __launch_bounds__(ROW_THREADS) ssm_ce_kernel(const SsmP P) {
    __shared__ float red[ROW_THREADS / 64];
    __shared__ float bc;
    const int b = blockIdx.x, tid = threadIdx.x, n1 = P.N + 1;
    float* row = P.logits + (long)b * n1;
    const int a = ssm_answer(P, b);
    // x_b0: the dot product in the same k order as the product tiles (sequential fmaf), one lane
    if (tid == 0) {
        const float* h = P.H + (long)b * P.ldh;
        const float* e = P.E + ssm_answer_row<GATHERED>(P, b) * P.d;
        float s = 0.f;
        for (int k = 0; k < P.d; ++k) s = fmaf(h[k], e[k], s);
        row[0] = s - ssm_corr(P, a);
    }
    __syncthreads();
    ssm_ce_row(row, P.dlogits + (long)b * n1, n1, P.inv_b, P.loss_rows + b, red, bc);
}

// roles by blockIdx.x: [0, tilesA) dE of candidate tiles (64 candidates x 64 dims), [tilesA, tilesA + tilesB) dh slabs
// (64 rows x 64 dims x slab), then dE of the answer columns (grid-stride over B d), and the last tilesM (0 unless a lazy Adam
// step of the plan) mark the step's touched item rows (lazy_mark_role)
template <bool GATHERED>
__global__ void __launch_bounds__(ROW_THREADS) ssm_bwd_kernel(const SsmP P) {
    __shared__ __attribute__((aligned(16))) float As[SSM_KS][SSM_LDP];
    __shared__ __attribute__((aligned(16))) float Bs[SSM_KS][SSM_LDP];
    __shared__ int it_s[SSM_TILE];             // the tile's candidate items (read only where rows are indexed by item)
    const int tid = threadIdx.x, B = P.B, d = P.d, n1 = P.N + 1, dt = (d + SSM_TILE - 1) / SSM_TILE;
    const int r0 = (tid >> 4) * 4, c0 = (tid & 15) * 4;
    int blk = blockIdx.x;
    if (blk < P.tilesA) {
        // dE[n_c][k] = sum_b g[b][1 + c] h_b[k]  (K = B in one workgroup: a fixed summation order)
        const int cand0 = (blk / dt) * SSM_TILE, k0 = (blk % dt) * SSM_TILE;
        if constexpr (!GATHERED) {
            if (tid < SSM_TILE) it_s[tid] = cand0 + tid < P.N ? P.cand[cand0 + tid] : 0;
            __syncthreads();
        }
        float acc[4][4] = {};
        ssm_tile<false, false>(B,
            [&](int k, int m) { return cand0 + m < P.N ? P.dlogits[(long)k * n1 + 1 + cand0 + m] : 0.f; },
            [&](int k, int m) { return k0 + m < d ? P.H[(long)k * P.ldh + k0 + m] : 0.f; }, As, Bs, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = r0 + i;
            if (cand0 + c >= P.N) continue;
            const long row = ssm_cand_row<GATHERED>(P, cand0 + c, it_s[c]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + c0 + j < d) ssm_grad<GATHERED>(P, row, k0 + c0 + j, acc[i][j]);
        }
        return;
    }
    blk -= P.tilesA;
    if (blk < P.tilesB) {
        // slab s: dh_b[k] = sum_{c in chunk s} g[b][1 + c] E[n_c][k]  (+ g[b][0] E[a_b][k] in slab 0)
        const int rt = (B + SSM_TILE - 1) / SSM_TILE;
        const int s = blk / (rt * dt), rem = blk % (rt * dt), row0 = (rem / dt) * SSM_TILE, k0 = (rem % dt) * SSM_TILE;
        const int cbeg = s * P.chunk, cend = min(P.N, cbeg + P.chunk);
        float acc[4][4] = {};
        for (int cb = cbeg; cb < cend; cb += SSM_TILE) {        // candidates in groups of 64: their items staged once
            const int cn = min(SSM_TILE, cend - cb);
            if constexpr (!GATHERED) {
                if (tid < SSM_TILE) it_s[tid] = tid < cn ? P.cand[cb + tid] : 0;
                __syncthreads();
            }
            ssm_tile<true, false>(cn,
                [&](int k, int m) { return row0 + m < B ? P.dlogits[(long)(row0 + m) * n1 + 1 + cb + k] : 0.f; },
                [&](int k, int m) { return k0 + m < d ? P.E[ssm_cand_row<GATHERED>(P, cb + k, it_s[k]) * d + k0 + m] : 0.f; },
                As, Bs, acc);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = row0 + r0 + i;
            if (b >= B) continue;
            float ga = 0.f;
            const float* ea = P.E;
            if (s == 0) {
                ga = P.dlogits[(long)b * n1];
                ea = P.E + ssm_answer_row<GATHERED>(P, b) * d;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + c0 + j;
                if (k >= d) continue;
                float v = acc[i][j];
                if (s == 0) v = fmaf(ga, ea[k], v);
                P.slab[(long)s * B * d + (long)b * d + k] = v;
            }
        }
        return;
    }
    blk -= P.tilesB;
    const int tilesC = gridDim.x - P.tilesA - P.tilesB - P.tilesM;
    if (blk >= tilesC) {
        lazy_mark_role(P.lazy, P.ids32, P.nids, P.answers, B, P.cand, P.N, P.V, 0, P.V, blk - tilesC, P.tilesM);
        return;
    }
    const long n = (long)B * d, nthr = (long)tilesC * ROW_THREADS;
    for (long e = (long)blk * ROW_THREADS + tid; e < n; e += nthr) {
        const int b = (int)(e / d), k = (int)(e % d);
        ssm_grad<GATHERED>(P, ssm_answer_row<GATHERED>(P, b), k, P.dlogits[(long)b * n1] * P.H[(long)b * P.ldh + k]);
    }
}

// The sharded step's draw, a launch of its own because the gather sits between it and the logits: one lane per draw writes
// cand[j], corr[j] of the step (key from the caller, step = state[1] read here); lane 0 resets the lazy row count of the step
// (null: dense Adam) before anything marks
__global__ void __launch_bounds__(ROW_THREADS) shard_ssm_draw_kernel(const SsmP P, uint64_t key, int* lazy_count) {
    const int j = blockIdx.x * ROW_THREADS + threadIdx.x;
    if (lazy_count && j == 0) *lazy_count = 0;
    if (j >= P.N) return;
    const int it = ssm_draw(P, (uint32_t)key, (uint32_t)(key >> 32), (uint32_t)P.state[1], j);
    P.cand[j] = it;
    P.corr[j] = ssm_corr(P, it);
}
