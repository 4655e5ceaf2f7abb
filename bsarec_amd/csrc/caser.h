// Convolution block of the Caser sibling model (bsarec_caser_fwd / bsarec_caser_bwd, include/bsarec_hip.h).  All arithmetic is fp32.
//   vertical    zv[b, c, j]   = sum_t Wv[c, t] x[b, t, j] + bv[c]                                    c < n_v
//   horizontal  c_h[b, f, t]  = sum_{i < h, j < d} Wh_h[f, i, j] x[b, t + i, j] + bh_h[f]            h = 1 .. L, t = 0 .. L - h
//               zh[b, h-1, f] = max(0, max_t c_h[b, f, t])
//   z = [zv | zh], F = n_v d + n_h L floats per sequence
//
// Forward, horizontal.  Height h is a product of M = L - h + 1 windows per sequence, K = h d, N = n_h, and row t of its left operand
// is x + t d with length h d: nothing is materialised.  A WAVE owns one (sequence, height): it walks the windows in groups of four
// 16-row tiles (v_mfma_f32_16x16x4_f32, the right-hand fragment of a k-block shared by the four tiles and, at n_h = 32, the left one
// by both column tiles), adds the bias, and keeps the running maximum and its t per lane; two exchanges across the four row groups
// of the lanes finish the maximum, so c_h never leaves registers.  Lane (l15, q) feeds k = 16 kb + 4 q + s in k-step (kb, s) to both
// operands (16-byte reads); a last k-block shorter than 16 feeds zeros.  A workgroup is four waves = four neighbouring sequences at
// one PAIR of heights (p + 1, L - p): the work of a height is h (L - h + 1), the same for both, and the four waves read the same
// filter rows at about the same time.  Tiles whose rows are all behind L - h are skipped; rows behind it inside a tile read zeros
// and are left out of the maximum.
//   One reduction order per (h, f): the k-steps run 0 .. K / 4 - 1 for every window, whatever its tile, row or sequence, and a row
// of an MFMA result depends on its own operand row alone.  So bit-identical windows give bit-identical c_h, the bits of a sequence do
// not depend on its batch, and the lowest t that attains the maximum is well defined: candidates are visited in rising t with a
// strict comparison, and the exchange prefers the lower t at equal value.  The winner is saved for the backward as an int per
// cell, -1 where the maximum is <= 0 (ReLU passes nothing).
// Forward, vertical: a thread owns four features of a sequence for all n_v filters, t rising.
//
// Backward.  One window per cell, so it is sparse and has no product worth an MFMA; every sum runs in a fixed order, no atomics:
//   caser_dx_kernel    a thread owns dx[b, t, 4 j4 ..]: the vertical terms c rising, then the cells (h, f) rising whose window
//                      covers t.  The cells' g and t* of the sequence are staged in LDS once per workgroup.
//   caser_dwh_kernel   a thread owns dWh_h[f, 4 e ..] (e over the h d / 4 quads of the filter) and adds g x[b, t* + .] over b rising;
//                      the first thread of a cell also writes dbh_h[f] = sum_b g.
//   caser_dv_kernel    a wave per (c, t): lane j4 sums dzv[b, c, .] x[b, t, .] over b rising, then a fixed shuffle tree; column
//                      t = L is dbv[c].  Its first workgroup writes 0 into the gaps of the flat gradient.
// A cell that passes nothing contributes g = 0 times a finite operand (the loops are branch-free so that their loads pipeline).
#pragma once
#include "common.h"

struct CaserP {
    const float* x;         // [B][L][d]
    const float* w;         // the flat weights
    float* z;               // [B][F]
    int* win;               // [B][L][n_h] winning t, -1: passes nothing; null: not kept
    int B, L, d, nh, nv;
    long F, bv_off, h_off;  // floats: conv_v.bias, conv_h.0.weight
};

// offset of conv_h.{h - 1}.weight [n_h][h][d]; its bias [n_h] follows it
__device__ __forceinline__ long caser_wh(const CaserP& P, int h) {
    return P.h_off + (long)P.nh * P.d * ((long)h * (h - 1) / 2) + (long)P.nh * (h - 1);
}

__device__ __forceinline__ f32x4 caser_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// grid ((L + 1) / 2 height pairs, ceil(B / 4)), 256 lanes; NT = column tiles of 16 filters
template <int NT>
__global__ void __launch_bounds__(256) caser_h_fwd_kernel(const CaserP P) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, q = lane >> 4;
    const int b = blockIdx.y * 4 + wave, L = P.L, d = P.d, nh = P.nh;
    if (b >= P.B) return;                                   // no barrier in this kernel
    const float* xb = P.x + (long)b * L * d;
    for (int pass = 0; pass < 2; ++pass) {
        const int h = pass == 0 ? (int)blockIdx.x + 1 : L - (int)blockIdx.x;
        if (pass == 1 && h <= (int)blockIdx.x + 1) break;   // the middle height of an odd L is its own partner
        const int T = L - h + 1, K = h * d;
        const float* Wh = P.w + caser_wh(P, h);
        const float* bias = Wh + (long)nh * K;
        float best[NT], bsv[NT];
        int bt[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            best[n] = -INFINITY;
            bt[n] = 0;
            bsv[n] = 16 * n + l15 < nh ? bias[16 * n + l15] : 0.f;
        }
        for (int t0 = 0; t0 < T; t0 += 64) {
            f32x4 acc[4][NT];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* xr[4];
            bool rv[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int t = t0 + 16 * m + l15;
                rv[m] = t < T;
                xr[m] = xb + (long)(rv[m] ? t : 0) * d;
            }
            for (int k0 = 0; k0 < K; k0 += 16) {
                const int k = k0 + 4 * q;
                const bool kv = k < K;
                f32x4 bf[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    bf[n] = kv && 16 * n + l15 < nh ? ld4(Wh + (long)(16 * n + l15) * K + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    if (t0 + 16 * m >= T) continue;         // wave-uniform: the whole tile is behind the last window
                    const f32x4 af = kv && rv[m] ? ld4(xr[m] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int n = 0; n < NT; ++n) acc[m][n] = caser_mfma(af[s], bf[n][s], acc[m][n]);
                }
            }
            // register i of tile m: window t0 + 16 m + 4 q + i, filter 16 n + l15; rising t inside a lane
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int t = t0 + 16 * m + 4 * q + i;
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const float v = acc[m][n][i] + bsv[n];
                        if (t < T && v > best[n]) { best[n] = v; bt[n] = t; }
                    }
                }
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                const float v2 = __shfl_xor(best[n], off);
                const int t2 = __shfl_xor(bt[n], off);
                if (v2 > best[n] || (v2 == best[n] && t2 < bt[n])) { best[n] = v2; bt[n] = t2; }
            }
            const int f = 16 * n + l15;
            if (q == 0 && f < nh) {
                const bool pass_g = best[n] > 0.f;
                P.z[(long)b * P.F + (long)P.nv * d + (long)(h - 1) * nh + f] = pass_g ? best[n] : 0.f;
                if (P.win) P.win[((long)b * L + (h - 1)) * nh + f] = pass_g ? bt[n] : -1;
            }
        }
    }
}

// grid ceil(B d / 4 / 256), 256 lanes
__global__ void __launch_bounds__(256) caser_v_fwd_kernel(const CaserP P) {
    const int d4 = P.d >> 2, L = P.L, nv = P.nv;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)P.B * d4) return;
    const long b = e / d4;
    const int j = (int)(e - b * d4) << 2;
    const float* xp = P.x + b * L * P.d + j;
    f32x4 acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < L; ++t) {
        const f32x4 xv = ld4(xp + (long)t * P.d);
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c < nv) acc[c] += P.w[c * L + t] * xv;
    }
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (c < nv) st4(P.z + b * P.F + (long)c * P.d + j, acc[c] + P.w[P.bv_off + c]);
}

struct CaserBwdP {
    const float* x;         // [B][L][d]
    const float* w;
    const float* dz;        // [B][F]
    const int* win;         // [B][L][n_h]
    float* dx;              // [B][L][d]
    float* dw;              // the flat gradient
    int B, L, d, nh, nv;
    long F, bv_off, h_off;
};

__device__ __forceinline__ long caser_wh(const CaserBwdP& P, int h) {
    return P.h_off + (long)P.nh * P.d * ((long)h * (h - 1) / 2) + (long)P.nh * (h - 1);
}

// grid (B, ceil(L d / 4 / 256)), 256 lanes, dynamic LDS L n_h (4 + 2) bytes
__global__ void __launch_bounds__(256) caser_dx_kernel(const CaserBwdP P) {
    extern __shared__ __attribute__((aligned(16))) float caser_lds[];
    const int L = P.L, d = P.d, nh = P.nh, d4 = d >> 2, cells = L * nh;
    float* gs = caser_lds;
    short* ts = reinterpret_cast<short*>(caser_lds + cells);
    const long b = blockIdx.x;
    const float* dzb = P.dz + b * P.F;
    for (int c = threadIdx.x; c < cells; c += 256) {
        const int w = P.win[b * cells + c];
        gs[c] = w >= 0 ? dzb[(long)P.nv * d + c] : 0.f;
        ts[c] = (short)w;
    }
    __syncthreads();
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= L * d4) return;
    const int t = e / d4, j = (e - t * d4) << 2;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < P.nv; ++c) acc += P.w[c * L + t] * ld4(dzb + (long)c * d + j);
    for (int h = 1; h <= L; ++h) {
        const float* Wh = P.w + caser_wh(P, h) + j;
        const long K = (long)h * d;
#pragma unroll 4
        for (int f = 0; f < nh; ++f) {
            const int ws = ts[(h - 1) * nh + f], i = t - ws;
            const bool in = ws >= 0 && i >= 0 && i < h;
            const float g = in ? gs[(h - 1) * nh + f] : 0.f;
            acc += g * ld4(Wh + f * K + (long)(in ? i : 0) * d);
        }
    }
    st4(P.dx + (b * L + t) * d + j, acc);
}

// grid (L n_h cells, ceil(L d / 4 / 256)), 256 lanes
__global__ void __launch_bounds__(256) caser_dwh_kernel(const CaserBwdP P) {
    const int L = P.L, d = P.d, nh = P.nh, cells = L * nh;
    const int cell = blockIdx.x, h = cell / nh + 1, f = cell - (h - 1) * nh;
    const int K4 = h * (d >> 2);
    if ((int)blockIdx.y * 256 >= K4) return;                // workgroup-uniform
    const int e = blockIdx.y * 256 + threadIdx.x;
    const bool on = e < K4;
    const float* xe = P.x + 4 * (on ? e : 0);
    const float* gz = P.dz + (long)P.nv * d + cell;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float gsum = 0.f;
#pragma unroll 8
    for (int b = 0; b < P.B; ++b) {
        const int ws = P.win[(long)b * cells + cell];
        const float g = ws >= 0 ? gz[(long)b * P.F] : 0.f;
        gsum += g;
        acc += g * ld4(xe + ((long)b * L + (ws >= 0 ? ws : 0)) * d);
    }
    float* dW = P.dw + caser_wh(P, h);
    if (on) st4(dW + (long)f * 4 * K4 + 4 * e, acc);
    if (e == 0) dW[(long)nh * 4 * K4 + f] = gsum;
}

// grid (L + 1, n_v), 64 lanes
__global__ void __launch_bounds__(64) caser_dv_kernel(const CaserBwdP P) {
    const int L = P.L, d = P.d, t = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    float acc = 0.f;
    if (4 * lane < d) {
        const float* gz = P.dz + (long)c * d + 4 * lane;
        const float* xp = P.x + (long)(t < L ? t : 0) * d + 4 * lane;
#pragma unroll 8
        for (int b = 0; b < P.B; ++b) {
            const f32x4 g = ld4(gz + (long)b * P.F);
            if (t < L) {
                const f32x4 xv = ld4(xp + (long)b * L * d);
                acc += ((g[0] * xv[0] + g[1] * xv[1]) + g[2] * xv[2]) + g[3] * xv[3];
            } else {
                acc += (g[0] + g[1]) + (g[2] + g[3]);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) P.dw[t < L ? (long)c * L + t : P.bv_off + c] = acc;
    if (t == 0 && c == 0) {                                 // the gaps behind conv_v.weight and conv_v.bias (the other tensors have none)
        for (long i = (long)P.nv * L + lane; i < P.bv_off; i += 64) P.dw[i] = 0.f;
        for (long i = P.bv_off + P.nv + lane; i < P.h_off; i += 64) P.dw[i] = 0.f;
    }
}
