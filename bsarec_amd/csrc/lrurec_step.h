// The row kernels of the LRURec training step (bsarec_lrurec_loss_grad / bsarec_lrurec_train_step, include/bsarec_hip.h): what the
// step needs between the pieces the library already has -- the recurrent layer (bsarec_lru_fwd / _bwd, lru.h), the feed-forward
// products with their epilogues (launch_gemm with EpiLinear / EpiLN and the grouped TN launch, epilogues.h), the LayerNorm
// backward (ln_bwd_kernel, kernels.h), the CE head (bsarec_ce_head_fwd / _bwd), the flush with the step's closing block
// (pair_flush_kernel, pair_step.h) and Adam.  Their host side is the block-model step of bsarec_hip.hip, which runs the Mamba4Rec
// step (bsarec_mamba4rec_*, the layer of mamba.h in the recurrent layer's place) through the same kernels.  All fp32; a row of d floats
// is held by LPR lanes, a float4 per lane, as in kernels.h (d <= 256, d % 4 == 0).  With T = B L rows and E [V][d]:
//   lrr_embed_kernel      x0[r, :] = Drop_0(LN(E[ids[r]])), xhat and rstd kept for the backward -- no position table; id 0 is an
//                         ordinary row (nn.Embedding without padding_idx), an id outside [0, V) reads a zero row.  Its lanes also
//                         clear the fixed-point accumulator of the item-table gradient (acc_clear) and write the 1.0f that the CE
//                         head's backward reads as d(loss), so a step does not depend on what the workspace holds on entry.
//   lrr_add_ln_kernel     a[r, :] = LN(Drop(z[r, :]) + x[r, :]), xhat and rstd kept: the LayerNorm behind the recurrent layer.
//   lrr_top_fill_kernel   the gradient entering the top block: dy[b, L - 1, :] = dh[b, :], zero elsewhere.
//   lrr_add_kernel        out = a + b: the recurrent layer's dx plus the residual gradient.
//   lrr_ln_sum_kernel     every LayerNorm's d(gamma) | d(beta) from the per-block partials of ln_bwd_kernel: G = 256 / (d / 2)
//                         thread groups per float4 column, group g adds blocks g, g + G, .. (four running sums, then
//                         (a0 + a1) + (a2 + a3)), and the groups' sums are added in group order through LDS -- one order, a
//                         function of the shape alone.  One workgroup per LayerNorm, all 2 N + 1 in one launch.
//   lrr_item_grad_kernel  the T lookup rows of the item-table gradient into the accumulator, through fix_scatter_block: row r adds
//                         de[r, :] (the embedding LayerNorm's backward, the dropout applied there) to row ids[r].
// Dropout is the Philox stream of common.h at element r d + c, i.e. oracle.dropout_keep(T d, p, seed, step, site); masks are
// regenerated wherever the backward needs them.  Every row statistic is an intra-wave sum in which all lanes take part (rows behind
// T and columns behind d add zeros), so the row loops are uniform over a workgroup.
#pragma once
#include "kernels.h"
#include "pair_step.h"

// xhat of a row and its rstd: TF-style LayerNorm (eps inside the root), the statistics over the d valid columns
template <int LPR>
__device__ __forceinline__ f32x4 lrr_row_norm(const f32x4 v, bool ok, int d, float eps, float& rs) {
    const float invd = 1.0f / (float)d;
    const float mean = group_sum<LPR>(v.x + v.y + v.z + v.w) * invd;
    f32x4 dl = {0.f, 0.f, 0.f, 0.f};
    if (ok) dl = v - mean;
    const float var = group_sum<LPR>(dl.x * dl.x + dl.y * dl.y + dl.z * dl.z + dl.w * dl.w) * invd;
    rs = 1.0f / sqrtf(var + eps);
    return dl * rs;
}

struct LrrEmbedP {
    const float* E; const int64_t* ids;
    const float* gamma; const float* beta; float eps;
    DropP drop;
    long T; int d, V;
    float* x; float* xhat; float* rstd;
    unsigned long long* acc; long acc_n2;       // the accumulator as pairs of 64-bit words, cleared here
    float* one;                                 // d(loss) = 1 of the CE head's backward
};

template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) lrr_embed_kernel(const LrrEmbedP P) {
    constexpr int RPP = ROW_THREADS / LPR;
    const int lr = threadIdx.x / LPR, lc = (threadIdx.x % LPR) << 2;
    const bool colok = lc < P.d;
    const DropSeed sd = drop_seed(P.drop);
    f32x4 g = {0.f, 0.f, 0.f, 0.f}, be = g;
    if (colok) { g = ld4(P.gamma + lc); be = ld4(P.beta + lc); }
    for (long r0 = (long)blockIdx.x * RPP; r0 < P.T; r0 += (long)gridDim.x * RPP) {
        const long r = r0 + lr;
        const bool ok = colok && r < P.T;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            const long id = P.ids[r];
            if (id >= 0 && id < P.V) v = ld4(P.E + id * P.d + lc);
        }
        float rs;
        const f32x4 xh = lrr_row_norm<LPR>(v, ok, P.d, P.eps, rs);
        if (ok) {
            const long e = r * P.d + lc;
            st4(P.xhat + e, xh);
            st4(P.x + e, (g * xh + be) * drop_mult4(P.drop, sd, (uint64_t)e >> 2));
            if (lc == 0) P.rstd[r] = rs;
        }
    }
    acc_clear(P.acc, P.acc_n2);
    if (blockIdx.x == 0 && threadIdx.x == 0) P.one[0] = 1.0f;
}

struct LrrAddLnP {
    const float* z; const float* x;
    const float* gamma; const float* beta; float eps;
    DropP drop;
    long T; int d;
    float* a; float* xhat; float* rstd;
};

template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) lrr_add_ln_kernel(const LrrAddLnP P) {
    constexpr int RPP = ROW_THREADS / LPR;
    const int lr = threadIdx.x / LPR, lc = (threadIdx.x % LPR) << 2;
    const bool colok = lc < P.d;
    const DropSeed sd = drop_seed(P.drop);
    f32x4 g = {0.f, 0.f, 0.f, 0.f}, be = g;
    if (colok) { g = ld4(P.gamma + lc); be = ld4(P.beta + lc); }
    for (long r0 = (long)blockIdx.x * RPP; r0 < P.T; r0 += (long)gridDim.x * RPP) {
        const long r = r0 + lr;
        const bool ok = colok && r < P.T;
        const long e = r * P.d + lc;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = ld4(P.z + e) * drop_mult4(P.drop, sd, (uint64_t)e >> 2) + ld4(P.x + e);
        float rs;
        const f32x4 xh = lrr_row_norm<LPR>(v, ok, P.d, P.eps, rs);
        if (ok) {
            st4(P.xhat + e, xh);
            st4(P.a + e, g * xh + be);
            if (lc == 0) P.rstd[r] = rs;
        }
    }
}

// dy [B][L][d4 float4] = dh [B][d4 float4] at t = L - 1, zero elsewhere; n4 = B L d4
__global__ void __launch_bounds__(ROW_THREADS) lrr_top_fill_kernel(const float* __restrict__ dh, float* __restrict__ dy, long n4,
                                                                   int L, int d4) {
    for (long i = (long)blockIdx.x * ROW_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * ROW_THREADS) {
        const long row = i / d4;
        const int c = (int)(i - row * d4);
        const long b = row / L;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row - b * L == L - 1) v = ld4(dh + (b * d4 + c) * 4);
        st4(dy + 4 * i, v);
    }
}

__global__ void __launch_bounds__(ROW_THREADS) lrr_add_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              float* __restrict__ out, long n4) {
    for (long i = (long)blockIdx.x * ROW_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * ROW_THREADS)
        st4(out + 4 * i, ld4(a + 4 * i) + ld4(b + 4 * i));
}

// part: [2 N + 1][gamma | beta][nb][d], LayerNorm j's partials as ln_bwd_kernel wrote them (j = 0 the embedding's, 1 + 2 k block
// k's behind the recurrent layer, 2 + 2 k its feed-forward's).  dw: the flat gradient; LayerNorm j's weight | bias stand at
// offset 0 (j = 0), first + k stride + at_layer or + at_ff.
struct LrrLnSumP {
    const float* part; int nb, d;
    float* dw; long first, stride, at_layer, at_ff;
};

__global__ void __launch_bounds__(ROW_THREADS) lrr_ln_sum_kernel(const LrrLnSumP P) {
    __shared__ f32x4 red[ROW_THREADS];
    const int j = blockIdx.x, k = (j - 1) >> 1;
    float* out = P.dw + (j == 0 ? 0 : P.first + k * P.stride + ((j & 1) ? P.at_layer : P.at_ff));
    const int Q = P.d / 2, G = ROW_THREADS / Q;              // float4 columns of gamma | beta (<= 128), thread groups (>= 2)
    const int q = threadIdx.x % Q, grp = threadIdx.x / Q;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    if (grp < G) {
        const int which = 4 * q >= P.d, c = 4 * q - which * P.d;     // d % 4 == 0: a float4 is inside gamma or inside beta
        const float* src = P.part + ((long)j * 2 + which) * P.nb * P.d + c;
        int s = grp;
        for (; s + 3 * G < P.nb; s += 4 * G) {                       // four loads in flight per thread
            a0 += ld4(src + (long)s * P.d);
            a1 += ld4(src + (long)(s + G) * P.d);
            a2 += ld4(src + (long)(s + 2 * G) * P.d);
            a3 += ld4(src + (long)(s + 3 * G) * P.d);
        }
        for (; s < P.nb; s += G) a0 += ld4(src + (long)s * P.d);
    }
    red[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (grp == 0) {
        f32x4 t = red[q];
        for (int g = 1; g < G; ++g) t += red[g * Q + q];
        st4(out + 4 * q, t);
    }
}

struct LrrItemGradP {
    const float* de; const int64_t* ids;        // [T][d], [T]
    long T; int d, V;
    unsigned long long* dA;                     // [V][d] fixed point
};

// grid ceil(T / CHUNK), CHUNK = SCATTER_FLOATS / (4 LPR) rows per block
template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) lrr_item_grad_kernel(const LrrItemGradP P) {
    __shared__ __attribute__((aligned(16))) float lds[fix_scatter_lds_bytes(LPR) / 4];
    fix_scatter_block<LPR>(P.T, P.d, P.dA, blockIdx.x, lds,
        [&](long r) { return pair_row_id(P.ids[r], P.V); },
        [&](long r, int lc) { return ld4(P.de + r * P.d + lc); });
}
