// fc1 of the Caser sibling model in both directions (bsarec_caser_fc_fwd / bsarec_caser_fc_bwd, and steps 4 and 6 of
// bsarec_caser_loss_grad / bsarec_caser_train_step, include/bsarec_hip.h).  All arithmetic is fp32, every product runs on
// v_mfma_f32_16x16x4_f32 (caser_mfma, caser.h).  With z [B, F] the convolution block's output, W1 [d, F], b1 [d]:
//   forward   m[b, k] = keep / (1 - p) of dropout site 0, stream element b F + k (oracle.dropout_keep(B F, p, seed, step, 0));
//             zd = z (.) m;  s = max(0, zd W1^T + b1)                                                              [B, d]
//   backward  du = ds where s > 0, else 0;  dW1 = du^T zd;  db1 = sum_b du;  dz = (du W1) (.) m                    [B, F]
// The mask: the forward leaves zd [B, F] in the workspace and the dW1 launch reads it -- zd is the right-hand operand of that
// product as it stands, so nothing is recomputed there; the dz launch regenerates m, one Philox call per float4 of dz, each float4
// owned by one lane.  With no mask (train = 0 or p = 0) zd IS z: nothing is stored and the backward reads z.  So every Philox group
// is evaluated exactly once per direction.
//
//   caser_fc_fwd_kernel<NT, NW>  one workgroup of NW waves per 16-row tile (NW = 8 for d <= 128, 4 above: the partial tiles of
//                            NW - 1 waves must fit in 64 KB of LDS).  Wave w takes the w-th NW-th of the k-blocks of 16 (a
//                            function of F and d alone) for ALL column tiles of 16 (NT <= 16 accumulators), so the float4 of z a lane
//                            loads -- and its Philox call -- serves every column tile.  Waves 1.. leave their partial tiles in LDS;
//                            wave 0 adds them in wave order, then the bias, applies the ReLU and stores.  Lane (l15, q) feeds
//                            k = 16 kb + 4 q + i in k-step (kb, i) to both operands (16-byte reads).
//   caser_fc_dz_kernel       a wave owns 16 rows x 64 features, K = d.  The four column tiles are INTERLEAVED: column l15 of tile t
//                            is feature f0 + 4 l15 + t, so that a lane's right-hand fragment of a k is one float4 of a W1 row
//                            and its four results of a row are one float4 of dz: one Philox call, one 16-byte store.
//   caser_fc_dw_kernel       a workgroup of four waves owns dW1[j0 .. j0 + 63][f0 .. f0 + 63] (4 x 4 tiles, rows and columns
//                            interleaved as above: one float4 of du[b] and one of zd[b] per lane and k-step feed 16 MFMAs), K = B.
//                            Wave w takes the w-th quarter of the batch (multiples of 4 rows, a function of B alone), b rising;
//                            partial tiles are added in wave order through LDS.  The workgroups of the first feature tile also
//                            form db1[j0 .. j0 + 63] with the same split.
// One order per sum, a function of the shape alone; no atomics.  A row of an MFMA result depends on its own operand row alone, and
// the K split of the forward does not depend on B: a row of s has the same bits whatever the batch around it.
// Rows behind B, columns behind d or F and k behind the K of a product read zeros through a clamped address; nothing out of range
// is loaded or stored (d and F are multiples of 4, so a float4 is inside or outside as a whole).
#pragma once
#include "caser.h"

struct CaserFcP {
    const float* z;         // [B][F]
    const float* zd;        // [B][F] what the backward multiplies du by: the workspace copy, or z when there is no mask
    float* zd_out;          // forward: where z (.) m goes; null: not kept
    const float* w;         // W1 [d][F], then b1 [d]
    const float* s;         // [B][d] (backward)
    const float* ds;        // [B][d]
    float* s_out;           // [B][d] (forward)
    float* dz;              // [B][F]
    float* dw;              // dW1 [d][F], then db1 [d]
    int B, F, d;
    DropP drop;
};

constexpr int CASER_FC_LDS_PAD = 4;     // floats between the rows of a partial tile in LDS

// grid ceil(B / 16), 64 NW lanes, dynamic LDS (NW - 1) * 16 * (16 NT + 4) floats
template <int NT, int NW>
__global__ void __launch_bounds__(64 * NW) caser_fc_fwd_kernel(const CaserFcP P) {
    extern __shared__ __attribute__((aligned(16))) float caser_fc_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, q = lane >> 4;
    const int F = P.F, d = P.d, b0 = blockIdx.x * 16;
    const DropSeed sd = drop_seed(P.drop);
    const int nkb = (F + 15) >> 4, per = (nkb + NW - 1) / NW;
    const int kb_lo = wave * per, kb_hi = min(kb_lo + per, nkb);
    const int row = b0 + l15;
    const bool rv = row < P.B;
    const long zoff = (long)(rv ? row : 0) * F;
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = kb_lo; kb < kb_hi; ++kb) {
        const int k = 16 * kb + 4 * q;
        const bool kv = k < F;
        f32x4 af = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kv && rv) {
            af = ld4(P.z + zoff + k) * drop_mult4(P.drop, sd, (uint64_t)(zoff + k) >> 2);
            if (P.zd_out) st4(P.zd_out + zoff + k, af);
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            if (16 * n >= d) continue;                      // wave-uniform
            const int col = 16 * n + l15;
            const f32x4 bf = kv && col < d ? ld4(P.w + (long)col * F + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[n] = caser_mfma(af[i], bf[i], acc[n]);
        }
    }
    // register i of tile n: row 4 q + i, column 16 n + l15
    const int ldr = 16 * NT + CASER_FC_LDS_PAD;
    if (wave > 0) {
        float* part = caser_fc_lds + (long)(wave - 1) * 16 * ldr;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int i = 0; i < 4; ++i) part[(4 * q + i) * ldr + 16 * n + l15] = acc[n][i];
    }
    __syncthreads();
    if (wave > 0) return;
    const float* bias = P.w + (long)d * F;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int col = 16 * n + l15;
        if (col >= d) continue;
        const float bv = bias[col];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = b0 + 4 * q + i;
            float v = acc[n][i];
#pragma unroll
            for (int w = 0; w < NW - 1; ++w) v += caser_fc_lds[((long)w * 16 + 4 * q + i) * ldr + col];
            v += bv;
            if (r < P.B) P.s_out[(long)r * d + col] = v > 0.f ? v : 0.f;
        }
    }
}

// du[b, j .. j + 3]: ds where s > 0
__device__ __forceinline__ f32x4 caser_fc_du4(const CaserFcP& P, long e) {
    const f32x4 sv = ld4(P.s + e), g = ld4(P.ds + e);
    return f32x4{sv[0] > 0.f ? g[0] : 0.f, sv[1] > 0.f ? g[1] : 0.f, sv[2] > 0.f ? g[2] : 0.f, sv[3] > 0.f ? g[3] : 0.f};
}

// grid (ceil(F / 256), ceil(B / 16)), 256 lanes = four waves of 64 features each; no barrier
__global__ void __launch_bounds__(256) caser_fc_dz_kernel(const CaserFcP P) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, q = lane >> 4;
    const int F = P.F, d = P.d, b0 = blockIdx.y * 16;
    const int f0 = (blockIdx.x * 4 + wave) * 64;
    if (f0 >= F) return;
    const DropSeed sd = drop_seed(P.drop);
    const int row = b0 + l15, f = f0 + 4 * l15;
    const bool rv = row < P.B, fv = f < F;
    const long uoff = (long)(rv ? row : 0) * d;
    const float* wp = P.w + (fv ? f : 0);
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < d; k0 += 16) {
        const int k = k0 + 4 * q;
        const bool kv = k < d;
        const f32x4 af = kv && rv ? caser_fc_du4(P, uoff + k) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bf[i] = kv && fv ? ld4(wp + (long)(k + i) * F) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = caser_mfma(af[i], bf[i][t], acc[t]);
    }
    // register i of tile t: row 4 q + i, feature f0 + 4 l15 + t
    if (!fv) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = b0 + 4 * q + i;
        if (r >= P.B) continue;
        const long e = (long)r * F + f;
        st4(P.dz + e, f32x4{acc[0][i], acc[1][i], acc[2][i], acc[3][i]} * drop_mult4(P.drop, sd, (uint64_t)e >> 2));
    }
}

// the rows of wave w: [lo, hi), multiples of 4 except the end
__device__ __forceinline__ void caser_fc_bsplit(int B, int wave, int& lo, int& hi) {
    const int per = (((B + 3) >> 2) + 3) >> 2 << 2;
    lo = min(wave * per, B);
    hi = min(lo + per, B);
}

// grid (ceil(F / 64), ceil(d / 64)), 256 lanes
__global__ void __launch_bounds__(256) caser_fc_dw_kernel(const CaserFcP P) {
    __shared__ __attribute__((aligned(16))) float part[3][16][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, q = lane >> 4;
    const int F = P.F, d = P.d, B = P.B;
    const int f0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
    const int f = f0 + 4 * l15, j = j0 + 4 * l15;
    const bool fv = f < F, jv = j < d;
    int lo, hi;
    caser_fc_bsplit(B, wave, lo, hi);
    f32x4 acc[4][4];                                        // [row tile s][column tile t]
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int bb = lo; bb < hi; bb += 4) {
        const int b = bb + q;
        const bool bv = b < hi;
        const f32x4 af = bv && jv ? caser_fc_du4(P, (long)b * d + j) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 bf = bv && fv ? ld4(P.zd + (long)b * F + f) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[s][t] = caser_mfma(af[s], bf[t], acc[s][t]);
    }
    // db1 of the first feature tile: lane `lane` of wave w sums column j0 + lane over the wave's rows, b rising
    const bool with_bias = blockIdx.x == 0;
    float bsum = 0.f;
    if (with_bias && j0 + lane < d)
        for (int b = lo; b < hi; ++b) {
            const long e = (long)b * d + j0 + lane;
            bsum += P.s[e] > 0.f ? P.ds[e] : 0.f;
        }
    if (wave > 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) st4(&part[wave - 1][4 * s + t][0][0] + 4 * lane, acc[s][t]);
    }
    __syncthreads();
    float* bred = &part[0][0][0][0];
    if (wave == 0) {
        // register i of tile (s, t): row j0 + 4 (4 q + i) + s, feature f0 + 4 l15 + t
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            f32x4 v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                v[t] = acc[s][t];
#pragma unroll
                for (int w = 0; w < 3; ++w) v[t] += ld4(&part[w][4 * s + t][0][0] + 4 * lane);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = j0 + 4 * (4 * q + i) + s;
                if (fv && r < d) st4(P.dw + (long)r * F + f, f32x4{v[0][i], v[1][i], v[2][i], v[3][i]});
            }
        }
    }
    if (!with_bias) return;                                 // workgroup-uniform
    __syncthreads();
    if (wave > 0) bred[(wave - 1) * 64 + lane] = bsum;
    __syncthreads();
    if (wave == 0 && j0 + lane < d) P.dw[(long)d * F + j0 + lane] = ((bsum + bred[lane]) + bred[64 + lane]) + bred[128 + lane];
}
