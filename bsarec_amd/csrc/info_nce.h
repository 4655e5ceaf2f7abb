// DuoRec's contrastive head (bsarec_info_nce_fwd / bsarec_info_nce_bwd, include/bsarec_hip.h): InfoNCE over the n = 2B rows
// z = [z_i; z_j] without the n x n score matrix.  u_r = z_r (dot) or z_r / max(|z_r|, 1e-8) (cos); s_rc = u_r . u_c / tau;
// lse_r = log sum_{c != r} exp(s_rc); row_r = lse_r - s_{r, pos(r)}, pos(r) = (r + B) mod n; loss = mean_r row_r.
//
// Launch shape.  Scores are formed in 64 x 64 tiles by one 256-lane workgroup: register-tiled fp32 FMA, each lane a 4 x 4
// block (rows ty + 16 i, keys tx + 16 j), both operands read from LDS as float4 along k (2 ds_read_b128 per 16 FMAs, the
// ratio of ssm_tile).  A score is FOUR partial sums (k mod 4) added as (x + y) + (z + w): a quarter of the chain length of
// one fmaf chain, and the same bits wherever the score is formed -- forward, backward, (r, c) and (c, r).
// The grid is (key splits S, row tiles T), T = ceil(n / 64) and S = min(T, ceil(256 / T), 8): B = 256 gives 8 x 8 = 64 single-tile
// workgroups instead of 8 that walk 8 tiles each; B = 1024 gives 8 x 32.  A split owns a contiguous range of key tiles.
//   forward:  nce_norm_kernel (cos only: the clamped norms)
//             nce_fwd_kernel  per (split, row tile): an online (max, sum) per lane, merged over the 16 lanes of a row by a
//                             shuffle butterfly, one (m, l) per (split, row); the lane that holds column pos(r) stores s_pos
//             nce_stat_kernel one workgroup: merges the S partials of a row in split order -> lse, rows_out; the mean in a
//                             fixed order (lane-strided sums, then mean_of_1024's LDS tree) -> loss_out
//   backward: nce_bwd_kernel  per (split, row tile): the score tile again, W_rc = exp(s - lse_r) + exp(s - lse_c) through
//                             LDS, acc[64 x d] += W . u_keys (lanes re-mapped to rows 4 ty + i, columns 4 tx + j of a 64-column
//                             chunk of d, W read k-major), stored to the split's slab
//             nce_dz_kernel   one wave per row: the slabs added in split order, - 2 u_pos, * g / (n tau), the cos projection
// No atomics, no host synchronisation, no allocation; every sum has one order, so results are bit-deterministic.
// Workspace (floats): lse[n] | s_pos[n] | norm[n] | m[S][n] | l[S][n] | pad to 4 | slab[S][n][d] -- linear in B (S n <= 16384 + n).
#pragma once
#include "kernels.h"

#define NCE_TILE 64
#define NCE_LDP 68                           // LDS row stride in floats: 64 + one float4, so 16 lanes' float4 reads spread over all banks
#define NCE_EPS 1e-8f                        // torch.nn.functional.cosine_similarity's clamp of each norm

struct NceP {
    const float* zi; const float* zj;        // [B, d] with row strides ldi, ldj
    long ldi, ldj;
    int B, n, d, cos, S, T;
    float inv_tau;
    float *lse, *spos, *norm, *pm, *pl, *slab;   // the workspace
};

static inline int nce_splits(int n) {
    const int T = (n + NCE_TILE - 1) / NCE_TILE;
    int S = (256 + T - 1) / T;
    if (S > T) S = T;
    return S > 8 ? 8 : S;
}
// floats in front of the slabs (a multiple of 4: the slabs are written as float4), and in all
static inline long nce_stat_floats(long n, long S) { return (3 * n + 2 * S * n + 3) / 4 * 4; }
static inline long nce_workspace_floats(int B, int d) {
    const long n = 2L * B, S = nce_splits((int)n);
    return nce_stat_floats(n, S) + S * n * d;
}

__device__ __forceinline__ const float* nce_row(const NceP& P, int r) {
    return r < P.B ? P.zi + (long)r * P.ldi : P.zj + (long)(r - P.B) * P.ldj;
}
// 1 / the clamped norm of row r (1 for dot)
__device__ __forceinline__ float nce_scale(const NceP& P, int r) { return P.cos ? 1.0f / P.norm[r] : 1.0f; }

// Rows [r0, r0 + 64) x columns [k0, k0 + 64) of u into dst[64][NCE_LDP]; zeros outside n x d.
__device__ __forceinline__ void nce_stage(const NceP& P, int r0, int k0, float (*dst)[NCE_LDP]) {
    for (int x = threadIdx.x; x < NCE_TILE * 16; x += ROW_THREADS) {
        const int m = x >> 4, c = (x & 15) << 2, r = r0 + m;
        f32x4 v = {0, 0, 0, 0};
        if (r < P.n && k0 + c < P.d) v = ld4(nce_row(P, r) + k0 + c) * nce_scale(P, r);
        st4(&dst[m][c], v);
    }
}

// s[i][j] = u_(r0 + ty + 16 i) . u_(c0 + tx + 16 j) * inv_tau.  Ends behind a barrier: Qs / Ks may be written again.  With
// d <= 64 the row tile is staged once (q_ready) and Ks holds the key tile's whole rows on return.
__device__ __forceinline__ void nce_scores(const NceP& P, int r0, int c0, float (*Qs)[NCE_LDP], float (*Ks)[NCE_LDP], bool q_ready,
                                           float s[4][4]) {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
    for (int k0 = 0; k0 < P.d; k0 += NCE_TILE) {
        if (k0 > 0) __syncthreads();
        if (!q_ready || P.d > NCE_TILE) nce_stage(P, r0, k0, Qs);
        nce_stage(P, c0, k0, Ks);
        __syncthreads();
        const int kend = P.d - k0 < NCE_TILE ? P.d - k0 : NCE_TILE;
#pragma unroll 4
        for (int k = 0; k < kend; k += 4) {
            f32x4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = ld4(&Qs[ty + 16 * i][k]); b[i] = ld4(&Ks[tx + 16 * i][k]); }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j].x = fmaf(a[i].x, b[j].x, acc[i][j].x); acc[i][j].y = fmaf(a[i].y, b[j].y, acc[i][j].y);
                    acc[i][j].z = fmaf(a[i].z, b[j].z, acc[i][j].z); acc[i][j].w = fmaf(a[i].w, b[j].w, acc[i][j].w);
                }
        }
    }
    __syncthreads();
    {   // contract(off): s is the ROUNDED product.  Fused into a caller's s - max or s - lse as fma(sum, inv_tau, -lse), it would
        // differ from the s that max and lse were made of by the product's rounding error (B = 1: lse = s exactly, W = 2 exactly)
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[i][j] = ((acc[i][j].x + acc[i][j].y) + (acc[i][j].z + acc[i][j].w)) * P.inv_tau;
    }
}

// clamped norms, one wave per row
__global__ void __launch_bounds__(ROW_THREADS) nce_norm_kernel(const NceP P) {
    const int r = blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= P.n) return;
    const float* z = nce_row(P, r);
    float q = 0.f;
    if (4 * lane < P.d) { const f32x4 v = ld4(z + 4 * lane); q = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
    if (lane == 0) P.norm[r] = fmaxf(sqrtf(q), NCE_EPS);
}

// grid (S, T)
__global__ void __launch_bounds__(ROW_THREADS) nce_fwd_kernel(const NceP P) {
    __shared__ __attribute__((aligned(16))) float Qs[NCE_TILE][NCE_LDP];
    __shared__ __attribute__((aligned(16))) float Ks[NCE_TILE][NCE_LDP];
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15, r0 = blockIdx.y * NCE_TILE;
    int t0, t1;
    split_range(blockIdx.x, P.T, P.S, t0, t1);              // this split's key tiles
    float m[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { m[i] = -INFINITY; l[i] = 0.f; }
    for (int t = t0; t < t1; ++t) {
        const int c0 = t * NCE_TILE;
        float s[4][4];
        nce_scores(P, r0, c0, Qs, Ks, t > t0, s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + ty + 16 * i;
            const int pos = r < P.B ? r + P.B : r - P.B;
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + tx + 16 * j;
                if (c >= P.n || c == r) s[i][j] = -INFINITY;
                if (c == pos && r < P.n) P.spos[r] = s[i][j];
                mx = fmaxf(mx, s[i][j]);
            }
            if (mx == -INFINITY) continue;
            const float M = fmaxf(m[i], mx);
            float add = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) add += expf(s[i][j] - M);
            l[i] = l[i] * expf(m[i] - M) + add;
            m[i] = M;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const float m2 = __shfl_xor(m[i], off, 64), l2 = __shfl_xor(l[i], off, 64);
            softmax_merge(m[i], l[i], m2, l2);
        }
        const int r = r0 + ty + 16 * i;
        if (tx == 0 && r < P.n) { P.pm[(long)blockIdx.x * P.n + r] = m[i]; P.pl[(long)blockIdx.x * P.n + r] = l[i]; }
    }
}

// one workgroup of 1024 lanes: lse, rows_out, loss
__global__ void __launch_bounds__(1024) nce_stat_kernel(const NceP P, float* __restrict__ loss_out, float* __restrict__ rows_out) {
    const int tid = threadIdx.x;
    float sum = 0.f;
    for (int r = tid; r < P.n; r += 1024) {
        const SoftmaxPart part = softmax_merge_splits(P, P.n, r);
        const float m = part.m, l = part.l;
        const float lse = m + logf(l);
        const float row = lse - P.spos[r];
        P.lse[r] = lse;
        if (rows_out) rows_out[r] = row;
        sum += row;
    }
    mean_of_1024(sum, P.n, loss_out);
}

// grid (S, T); NCH = ceil(d / 64) chunks of the output columns
template <int NCH>
__global__ void __launch_bounds__(ROW_THREADS) nce_bwd_kernel(const NceP P) {
    __shared__ __attribute__((aligned(16))) float Qs[NCE_TILE][NCE_LDP];
    __shared__ __attribute__((aligned(16))) float Ks[NCE_TILE][NCE_LDP];
    __shared__ __attribute__((aligned(16))) float Wt[NCE_TILE][NCE_LDP];     // Wt[key][row]
    __shared__ float lse_q[NCE_TILE], lse_k[NCE_TILE];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, r0 = blockIdx.y * NCE_TILE;
    int t0, t1;
    split_range(blockIdx.x, P.T, P.S, t0, t1);              // this split's key tiles
    if (tid < NCE_TILE) lse_q[tid] = r0 + tid < P.n ? P.lse[r0 + tid] : 0.f;
    float acc[NCH][4][4];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[c][i][j] = 0.f;
    for (int t = t0; t < t1; ++t) {
        const int c0 = t * NCE_TILE;
        if (tid < NCE_TILE) lse_k[tid] = c0 + tid < P.n ? P.lse[c0 + tid] : 0.f;       // read behind nce_scores' barriers
        float s[4][4];
        nce_scores(P, r0, c0, Qs, Ks, t > t0, s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = ty + 16 * i, r = r0 + m;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = tx + 16 * j, c = c0 + k;
                const bool on = r < P.n && c < P.n && c != r;
                Wt[k][m] = on ? expf(s[i][j] - lse_q[m]) + expf(s[i][j] - lse_k[k]) : 0.f;
            }
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (NCH > 1) {                                     // Ks holds one 64-column chunk at a time
                __syncthreads();
                nce_stage(P, c0, ch * NCE_TILE, Ks);
            }
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < NCE_TILE; ++k) {
                const f32x4 a = ld4(&Wt[k][4 * ty]), b = ld4(&Ks[k][4 * tx]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[ch][i][j] = fmaf(a[i], b[j], acc[ch][i][j]);
            }
        }
        __syncthreads();
    }
    float* slab = P.slab + (long)blockIdx.x * P.n * P.d;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + 4 * ty + i, c = ch * NCE_TILE + 4 * tx;
            if (r < P.n && c < P.d) st4(slab + (long)r * P.d + c, f32x4{acc[ch][i][0], acc[ch][i][1], acc[ch][i][2], acc[ch][i][3]});
        }
}

// one wave per row: du = g / (n tau) (sum_s slab_s - 2 u_pos); dot: dz = du; cos: dz = (du - u (u . du)) / |z|, or du / 1e-8
// for a row whose norm was clamped
__global__ void __launch_bounds__(ROW_THREADS) nce_dz_kernel(const NceP P, const float* __restrict__ gout, float* __restrict__ dzi,
                                                             float* __restrict__ dzj) {
    const int r = blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= P.n) return;
    const int pos = r < P.B ? r + P.B : r - P.B;
    const bool on = 4 * lane < P.d;
    const float coef = *gout * P.inv_tau / (float)P.n;
    f32x4 du = {0, 0, 0, 0}, u = {0, 0, 0, 0};
    if (on) {
        for (int s = 0; s < P.S; ++s) du += ld4(P.slab + ((long)s * P.n + r) * P.d + 4 * lane);
        du = (du - 2.0f * (ld4(nce_row(P, pos) + 4 * lane) * nce_scale(P, pos))) * coef;
    }
    if (P.cos) {
        const float nr = P.norm[r];
        if (nr > NCE_EPS) {
            if (on) u = ld4(nce_row(P, r) + 4 * lane) * (1.0f / nr);
            float p = (u.x * du.x + u.y * du.y) + (u.z * du.z + u.w * du.w);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) p += __shfl_xor(p, off, 64);
            du = (du - u * p) * (1.0f / nr);
        } else {
            du = du * (1.0f / NCE_EPS);
        }
    }
    if (on) st4((r < P.B ? dzi + (long)r * P.d : dzj + (long)(r - P.B) * P.d) + 4 * lane, du);
}
