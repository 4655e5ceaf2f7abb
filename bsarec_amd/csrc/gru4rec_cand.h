// GRU4Rec heads over candidates shared by the batch (bsarec_gru4rec_cand_head / _cand_loss_grad / _cand_train_step,
// include/bsarec_hip.h): every row b scores C candidates c_0 .. c_C-1 -- the batch's answers (candidates = 1, C = B) and behind them
// the loader's negatives (candidates = 2, C = 2 B) --, its positive is column b and its negatives are the columns whose item is not
// answers[b].  With s [B][d] the stack's output and r_bj = s_b . E[c_j]:
//   g4c_scores_kernel     R [B][C] in 64 x 64 tiles (ssm_tile of sampled_softmax.h: fp32 FMAs, the products are 3 B C d flops)
//   g4c_rows_kernel       one workgroup per row, the row staged in LDS once: the row's statistics, loss_b, and G_b = d(mean loss) /
//                         d(r_b) written in place of R_b (cross-entropy, TOP1 or BPR-max, the formulas at g4c_rows_kernel)
//   g4c_bwd_kernel        two roles in one grid: dEc [C][d] = G^T . s and ds [B][d] = G . E_c, each split over its summed dimension
//                         into nslab slabs (a function of the shape alone)
//   g4c_slab_sum_kernel   nslab > 1: the slabs added in slab order
//   g4c_item_grad_kernel  fix_scatter_block (kernels.h) over T + C rows: row r < T adds dx[r, :] * m to row ids[r] (the token rows
//                         of pair_item_grad_kernel, pair_token_row), row T + j adds dEc[j, :] to row c_j
// No floating-point atomics: every float sum has one order; the item-table rows are summed in 64-bit fixed point as
// pair_step.h describes.  An id outside [0, V) is never dereferenced: such a candidate is no column of any row (G = 0), and a
// row whose answer is outside has loss 0 and gradient 0.  The restatement in numpy is tests/gru4rec_cand_ref.py.
#pragma once
#include "pair_step.h"
#include "sampled_softmax.h"

#define G4C_MAX 8192                      // BSAREC_GRU4REC_CAND_MAX: the most candidate columns
#define G4C_CE 1
#define G4C_TOP1 2
#define G4C_BPR_MAX 3

struct Gru4RecCandP {
    const float* s; const float* E;       // [B][d], [V][d]
    const int64_t* ans; const int64_t* neg;
    int B, C, d, V, loss;
    float bpreg;
    float* R;                             // [B][C]: the scores, then G
    float* loss_rows;                     // [B]
    // g4c_bwd_kernel: slab q of dEc at outE + q strideE (rows b in [q chunkB, (q + 1) chunkB)), of ds at outS + q strideS (columns j
    // in [q chunkC, (q + 1) chunkC)); nslab == 1: the outputs themselves
    float* outE; float* outS; long strideE, strideS;
    int nslab, chunkB, chunkC, tilesA;
};

// candidate j's item, -1 outside [0, V); P: Gru4RecCandP, or the PairGradP of g4c_item_grad_kernel
template <class Params>
__device__ __forceinline__ int g4c_cand(const Params& P, int j) {
    return pair_row_id(j < P.B ? P.ans[j] : P.neg[j - P.B], P.V);
}

// grid (ceil(C / 64), ceil(B / 64)): rows = batch rows, columns = candidates
__global__ void __launch_bounds__(ROW_THREADS) g4c_scores_kernel(const Gru4RecCandP P) {
    __shared__ __attribute__((aligned(16))) float As[SSM_KS][SSM_LDP];
    __shared__ __attribute__((aligned(16))) float Bs[SSM_KS][SSM_LDP];
    __shared__ int it_s[SSM_TILE];
    const int tid = threadIdx.x, col0 = blockIdx.x * SSM_TILE, row0 = blockIdx.y * SSM_TILE;
    const int B = P.B, C = P.C, d = P.d;
    if (tid < SSM_TILE) it_s[tid] = col0 + tid < C ? g4c_cand(P, col0 + tid) : -1;
    __syncthreads();
    float acc[4][4] = {};
    ssm_tile<true, true>(d,
        [&](int k, int m) { return row0 + m < B ? P.s[(long)(row0 + m) * d + k] : 0.f; },
        [&](int k, int m) { return it_s[m] >= 0 ? P.E[(long)it_s[m] * d + k] : 0.f; }, As, Bs, acc);
    const int r0 = (tid >> 4) * 4, c0 = (tid & 15) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = row0 + r0 + i;
        if (b >= B) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (col0 + c0 + j < C) P.R[(long)b * C + col0 + c0 + j] = acc[i][j];
    }
}

// all-lanes sum / max of one 256-lane workgroup in one fixed order; red: ROW_THREADS / 64 floats of LDS, free again on return
__device__ __forceinline__ float g4c_block_sum(float v, float* red) {
    v = group_sum<64>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}
__device__ __forceinline__ float g4c_block_max(float v, float* red) {
    v = group_max<64>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return t;
}

// One workgroup per row b.  M = the columns j whose item is inside [0, V) and is not answers[b], m = |M|, x_j = r_bj, x_b the
// positive's score, sig' = sig (1 - sig), both from pair_sigmoid; inv = 1 / B:
//   ce       loss = logsumexp_{{b} + M} x - x_b;  G_j = (softmax_j - [j == b]) inv
//   top1     loss = (1 / m) sum_M [sig(x_j - x_b) + sig(x_j^2)];  G_j = (sig'(x_j - x_b) + 2 x_j sig'(x_j^2)) inv / m,
//            G_b = -sum_M sig'(x_j - x_b) inv / m.  x_j^2 = inf gives sig = 1 and sig' = 0 exactly.
//   bpr_max  p = softmax over M, A = sum p_j sig(x_b - x_j), Q = sum p_j x_j^2, S = sum p_j sig'(x_b - x_j);
//            loss = -log(A + 1e-10) + bpreg Q;  G_b = -S / (A + 1e-10) inv,
//            G_j = p_j [(sig'_j - (sig_j - A)) / (A + 1e-10) + bpreg (x_j^2 - Q + 2 x_j)] inv
// Every maximum is subtracted before an exp.  m = 0: loss 0 and a row of zeros.  Columns outside {b} + M get G = 0.
__global__ void __launch_bounds__(ROW_THREADS) g4c_rows_kernel(const Gru4RecCandP P) {
    __shared__ __attribute__((aligned(16))) float x[G4C_MAX];
    __shared__ unsigned char in_m[G4C_MAX];
    __shared__ float red[ROW_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, C = P.C;
    float* row = P.R + (long)b * C;
    const long ab = P.ans[b];
    const bool rowok = ab >= 0 && ab < P.V;
    float cnt = 0.f;
    for (int j = tid; j < C; j += ROW_THREADS) {
        const int c = g4c_cand(P, j);
        const bool m = rowok && c >= 0 && c != (int)ab;
        x[j] = row[j];
        in_m[j] = m ? 1 : 0;
        cnt += m ? 1.f : 0.f;
    }
    const float m = g4c_block_sum(cnt, red);             // exact: at most 8192 ones; the barriers inside publish x and in_m
    if (m == 0.f) {
        for (int j = tid; j < C; j += ROW_THREADS) row[j] = 0.f;
        if (tid == 0) P.loss_rows[b] = 0.f;
        return;
    }
    const float xb = x[b], inv = 1.0f / (float)P.B;
    if (P.loss == G4C_CE) {
        float mx = -INFINITY;
        for (int j = tid; j < C; j += ROW_THREADS) if (in_m[j] || j == b) mx = fmaxf(mx, x[j]);
        mx = g4c_block_max(mx, red);
        float z = 0.f;
        for (int j = tid; j < C; j += ROW_THREADS) if (in_m[j] || j == b) z += expf(x[j] - mx);
        const float lse = mx + logf(g4c_block_sum(z, red));
        for (int j = tid; j < C; j += ROW_THREADS)
            row[j] = (in_m[j] || j == b) ? (expf(x[j] - lse) - (j == b ? 1.0f : 0.0f)) * inv : 0.f;
        if (tid == 0) P.loss_rows[b] = lse - xb;
        return;
    }
    if (P.loss == G4C_TOP1) {
        const float w = inv / m;
        float ls = 0.f, us = 0.f;
        for (int j = tid; j < C; j += ROW_THREADS) {
            float g = 0.f;
            if (in_m[j]) {
                float sg, om, sq, oq;
                pair_sigmoid(x[j] - xb, sg, om);
                pair_sigmoid(x[j] * x[j], sq, oq);
                ls += sg + sq;
                us += sg * om;
                g = (sg * om + 2.0f * x[j] * (sq * oq)) * w;
            }
            if (j != b) row[j] = g;
        }
        ls = g4c_block_sum(ls, red);
        us = g4c_block_sum(us, red);
        if (tid == 0) { row[b] = -us * w; P.loss_rows[b] = ls / m; }
        return;
    }
    // BPR-max
    float mx = -INFINITY;
    for (int j = tid; j < C; j += ROW_THREADS) if (in_m[j]) mx = fmaxf(mx, x[j]);
    mx = g4c_block_max(mx, red);
    float z = 0.f, a = 0.f, q = 0.f, sp = 0.f;
    for (int j = tid; j < C; j += ROW_THREADS) {
        if (!in_m[j]) continue;
        const float e = expf(x[j] - mx);
        float sg, om;
        pair_sigmoid(xb - x[j], sg, om);
        z += e;
        a += e * sg;
        sp += e * (sg * om);
        if (e > 0.f) q += e * (x[j] * x[j]);            // a column of weight 0 adds nothing, whatever its square
    }
    z = g4c_block_sum(z, red);
    const float rz = 1.0f / z;                           // z >= 1: the maximum's column adds exp(0)
    a = g4c_block_sum(a, red) * rz;
    q = g4c_block_sum(q, red) * rz;
    sp = g4c_block_sum(sp, red) * rz;
    const float ra = 1.0f / (a + 1e-10f), lam = P.bpreg;
    for (int j = tid; j < C; j += ROW_THREADS) {
        float g = 0.f;
        if (in_m[j]) {
            const float p = expf(x[j] - mx) * rz;
            float sg, om;
            pair_sigmoid(xb - x[j], sg, om);
            if (p > 0.f) g = p * ((sg * om - (sg - a)) * ra + lam * (x[j] * x[j] - q + 2.0f * x[j])) * inv;
        }
        if (j != b) row[j] = g;
    }
    if (tid == 0) { row[b] = -sp * ra * inv; P.loss_rows[b] = -logf(a + 1e-10f) + lam * q; }
}

// roles by blockIdx.x: [0, tilesA) slab q of dEc (64 candidates x 64 dims, summed over the rows of the slab), behind them slab q of
// ds (64 rows x 64 dims, summed over the candidates of the slab).  A slab behind the end of its range is written as zeros.
__global__ void __launch_bounds__(ROW_THREADS) g4c_bwd_kernel(const Gru4RecCandP P) {
    __shared__ __attribute__((aligned(16))) float As[SSM_KS][SSM_LDP];
    __shared__ __attribute__((aligned(16))) float Bs[SSM_KS][SSM_LDP];
    __shared__ int it_s[SSM_TILE];
    const int tid = threadIdx.x, B = P.B, C = P.C, d = P.d, dt = (d + SSM_TILE - 1) / SSM_TILE;
    const int r0 = (tid >> 4) * 4, c0 = (tid & 15) * 4;
    int blk = blockIdx.x;
    float acc[4][4] = {};
    if (blk < P.tilesA) {
        // dEc[j][k] = sum_b G[b][j] s_b[k]
        const int ct = (C + SSM_TILE - 1) / SSM_TILE;
        const int q = blk / (ct * dt), rem = blk % (ct * dt), cand0 = (rem / dt) * SSM_TILE, k0 = (rem % dt) * SSM_TILE;
        const int bbeg = min(B, q * P.chunkB), bend = min(B, bbeg + P.chunkB);
        ssm_tile<false, false>(bend - bbeg,
            [&](int k, int m) { return cand0 + m < C ? P.R[(long)(bbeg + k) * C + cand0 + m] : 0.f; },
            [&](int k, int m) { return k0 + m < d ? P.s[(long)(bbeg + k) * d + k0 + m] : 0.f; }, As, Bs, acc);
        float* out = P.outE + (long)q * P.strideE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = cand0 + r0 + i;
            if (j >= C) continue;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (k0 + c0 + jj < d) out[(long)j * d + k0 + c0 + jj] = acc[i][jj];
        }
        return;
    }
    blk -= P.tilesA;
    // ds_b[k] = sum_j G[b][j] E[c_j][k]
    const int rt = (B + SSM_TILE - 1) / SSM_TILE;
    const int q = blk / (rt * dt), rem = blk % (rt * dt), row0 = (rem / dt) * SSM_TILE, k0 = (rem % dt) * SSM_TILE;
    const int cbeg = min(C, q * P.chunkC), cend = min(C, cbeg + P.chunkC);
    for (int cb = cbeg; cb < cend; cb += SSM_TILE) {            // candidates in groups of 64: their items staged once
        const int cn = min(SSM_TILE, cend - cb);
        if (tid < SSM_TILE) it_s[tid] = tid < cn ? g4c_cand(P, cb + tid) : -1;
        __syncthreads();
        ssm_tile<true, false>(cn,
            [&](int k, int m) { return row0 + m < B ? P.R[(long)(row0 + m) * C + cb + k] : 0.f; },
            [&](int k, int m) { return k0 + m < d && it_s[k] >= 0 ? P.E[(long)it_s[k] * d + k0 + m] : 0.f; }, As, Bs, acc);
    }
    float* out = P.outS + (long)q * P.strideS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = row0 + r0 + i;
        if (b >= B) continue;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            if (k0 + c0 + jj < d) out[(long)b * d + k0 + c0 + jj] = acc[i][jj];
    }
}

// dEc and ds out of their slabs, added in slab order; one float4 per lane, the groups of dEc first
__global__ void __launch_bounds__(ROW_THREADS) g4c_slab_sum_kernel(const float* slabE, const float* slabS, int nslab, long nE4,
                                                                   long nS4, float* dEc, float* ds) {
    const long i = (long)blockIdx.x * ROW_THREADS + threadIdx.x;
    if (i >= nE4 + nS4) return;
    const bool e = i < nE4;
    const long at = 4 * (e ? i : i - nE4), stride = 4 * (e ? nE4 : nS4);
    const float* src = (e ? slabE : slabS) + at;
    f32x4 v = ld4(src);
    for (int q = 1; q < nslab; ++q) v = v + ld4(src + q * stride);
    st4((e ? dEc : ds) + at, v);
}

// pair_item_grad_kernel with the head's rows read from dEc (PairGradP.head_rows): grid ceil((T + C) / CHUNK), CHUNK =
// SCATTER_FLOATS / (4 LPR)
template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) g4c_item_grad_kernel(const PairGradP P) {
    __shared__ __attribute__((aligned(16))) float lds[fix_scatter_lds_bytes(LPR) / 4];
    const long T = P.T;
    const DropSeed sd = drop_seed(P.drop);
    fix_scatter_block<LPR>(T + P.C, P.d, P.dA, blockIdx.x, lds,
        [&](long r) { return r < T ? pair_row_id(P.ids[r], P.V) : g4c_cand(P, (int)(r - T)); },
        [&](long r, int lc) { return r < T ? pair_token_row(P, sd, r, lc) : ld4(P.head_rows + (r - T) * P.d + lc); });
}
