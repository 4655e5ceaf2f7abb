// Band-limited autocorrelation attention of the FEARec sibling model (bsarec_fea_attn_fwd / bsarec_fea_attn_bwd,
// include/bsarec_hip.h).  All arithmetic is fp32; the band's impulse response is summed in fp64.
//
// The contract is written in the frequency domain: band DFTs of Q and K, the cross-spectrum S summed over channels, and
//   m[b, tau] = 1 / (D L) sum_{f in band} w_f Re(S[b, f] e^{+2 pi i f tau / L}).
// Every step of it is linear in the products Q[t, c] K[t', c], and collecting them gives the same number without a spectrum:
//   r[b, delta] = sum_{t, c} Q[b, t, c] K[b, (t + delta) mod L, c]                 (the diagonal sums of the Gram matrix Q K^T)
//   h[n]        = 1 / L sum_{f in band} w_f cos(2 pi f n / L)                      (the band's impulse response, even in n)
//   m[b, tau]   = 1 / D sum_delta r[b, delta] h[(delta + tau) mod L]
// (full band: h = [1, 0, ...] and m is the circular cross-correlation).  The kernels compute this form: one [L x D] . [D x L]
// product per sequence instead of two [2 nb x L] . [L x D] ones, no complex arithmetic, and the backward needs no spectra --
//   dQ[b, t, c]  = 1 / D sum_t' cv[b, (t' - t) mod L] K[b, t', c],   dK[b, t', c] = 1 / D sum_t cv[b, (t' - t) mod L] Q[b, t, c],
//   cv[b, n]     = sum_i dm[b, i] h[(n + idx_i) mod L]
// are products of a circulant [L x L] matrix, generated from L floats in LDS, with K and Q.  tests/fearec_ref.py states the
// frequency form; tests/test_fearec_cpu.py holds the two together.
//
// Launches (forward 3, in training mode 4; backward 3; one linear chain on the caller's stream):
//   fea_band_kernel     h[n] in fp64 from exact arguments (f n mod L), rounded once; L threads.
//   fea_corr_kernel     a workgroup per sequence: the Gram matrix in 16 x 16 tiles on v_mfma_f32_16x16x4_f32 (a wave owns a
//                       row tile and up to four column tiles: four independent accumulators that share the Q fragment), each
//                       tile folded onto its <= 31 delays through LDS in a fixed order (one pair of barriers per trip), the four waves' parts added in wave
//                       order, then m.  Evaluation mode: the top-k of m[b, .] by wave 0 in the same launch.
//   fea_select_kernel   training mode: g[tau] = sum_b m[b, tau] / B in a fixed order (four slices of b, added in slice order) and
//                       its top-k.
//   fea_shift_kernel    p = softmax(m[b, idx]) (forward; written once per sequence), out[b, t] = sum_i p_i V[b, (t + idx_i) mod L]
//                       in rising i, 16 bytes per lane.  The backward runs it on dOut with the shifts negated: dV.
//   fea_dp_kernel       dp[b, i] = <dOut[b], V[b] shifted by idx_i> (lane sums, a fixed shuffle tree, the waves in order), the
//                       softmax backward, cv[b, .].
//   fea_dqk_kernel      dQ and dK: a wave owns 16 rows x 64 channels; ONE 16-byte load of a row of K (or Q) feeds four MFMAs,
//                       whose column tiles interleave (tile n holds the channels 4 j + n), so a lane's four results are 16
//                       contiguous bytes of the output.
// The top-k takes the largest value k times; equal values go to the lower delay, within a lane by a strict comparison in rising
// tau and across lanes by comparing (value, tau).  No floating-point atomics, no cross-block waits; every sum has one order that
// is a function of the shape alone, and in evaluation mode nothing of a sequence depends on the rest of the batch.
#pragma once
#include "common.h"

struct FeaP {
    const float* q;         // [B][L][D]
    const float* k;
    const float* v;
    const float* dout;
    float* out;
    float* dq;
    float* dk;
    float* dv;
    float* m;               // [B][L]
    int* idx;               // train: [k]; eval: [B][k]
    float* p;               // [B][k]
    float* h;               // [L]
    float* cv;              // [B][L]
    int B, L, D, lo, hi, topk, train;
};

__device__ __forceinline__ f32x4 fea_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// grid 1, 256 lanes
__global__ void __launch_bounds__(256) fea_band_kernel(const FeaP P) {
    const int n = threadIdx.x, L = P.L;
    if (n >= L) return;
    double acc = 0.0;
    for (int f = P.lo; f < P.hi; ++f) {
        const int r = (int)(((long)f * n) % L);             // the argument reduced exactly: cospi(2 r / L)
        const double w = (f == 0 || 2 * f == L) ? 1.0 : 2.0;
        double c;
        if (r == 0) c = 1.0;
        else if (2 * r == L) c = -1.0;
        else if (4 * r == L || 4 * r == 3 * L) c = 0.0;
        else c = cospi(2.0 * (double)r / (double)L);
        acc += w * c;
    }
    P.h[n] = (float)(acc / (double)L);
}

// The k largest of vals[0 .. L) (LDS), ties to the lower index, written to out[0 .. k) in the order taken.  Wave 0 calls it with
// all 64 lanes; L <= 256, 1 <= k <= min(L, 32).
__device__ __forceinline__ void fea_topk_wave(const float* vals, int L, int k, int lane, int* out) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = lane + 64 * j < L ? vals[lane + 64 * j] : -INFINITY;
    bool taken[4] = {false, false, false, false};
    for (int i = 0; i < k; ++i) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;                                // a lane with nothing left offers (-inf, no index)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool can = lane + 64 * j < L && !taken[j];
            if (can && (bi == 0x7fffffff || v[j] > bv)) { bv = v[j]; bi = lane + 64 * j; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float v2 = __shfl_xor(bv, off);
            const int i2 = __shfl_xor(bi, off);
            const bool mine = bi != 0x7fffffff, theirs = i2 != 0x7fffffff;
            if (theirs && (!mine || v2 > bv || (v2 == bv && i2 < bi))) { bv = v2; bi = i2; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (bi == lane + 64 * j) taken[j] = true;
        if (lane == 0) out[i] = bi;
    }
}

// grid B, 256 lanes
__global__ void __launch_bounds__(256) fea_corr_kernel(const FeaP P) {
    __shared__ float tile[4][4][16][17];                    // [wave][column tile]: a wave's patch is its own
    __shared__ float rw[4][256];
    __shared__ float hs[256], rs[256], ms[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q = lane >> 4;
    const int L = P.L, D = P.D, nT = (L + 15) >> 4, nG = (nT + 3) >> 2;
    const long b = blockIdx.x;
    const float* Qb = P.q + b * L * D;
    const float* Kb = P.k + b * L * D;
    hs[tid] = tid < L ? P.h[tid] : 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) rw[w][tid] = 0.f;
    __syncthreads();
    const int items = nT * nG, trips = (items + 3) >> 2;    // the same trip count in every wave: the loop holds barriers
    const int nd = L < 31 ? L : 31;
    for (int trip = 0; trip < trips; ++trip) {
        const int it = trip * 4 + wave;
        const bool on = it < items;
        const int tr = on ? it / nG : 0, cg = on ? it - tr * nG : 0;
        f32x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (on) {
            const int ta = 16 * tr + l15;
            const float* qa = Qb + (long)(ta < L ? ta : 0) * D;
            const float* kb[4];
            bool kv[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int tb = 16 * (4 * cg + n) + l15;
                kv[n] = tb < L;
                kb[n] = Kb + (long)(kv[n] ? tb : 0) * D;
            }
            for (int k0 = 0; k0 < D; k0 += 16) {
                const int kk = k0 + 4 * q;
                const bool kin = kk < D;
                const f32x4 af = kin && ta < L ? ld4(qa + kk) : f32x4{0.f, 0.f, 0.f, 0.f};
                f32x4 bf[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) bf[n] = kin && kv[n] ? ld4(kb[n] + kk) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int n = 0; n < 4; ++n) acc[n] = fea_mfma(af[s], bf[n][s], acc[n]);
            }
        }
        // register i of tile n: G[16 tr + 4 q + i][16 (4 cg + n) + l15]; the four tiles go to LDS between one pair of barriers
        // and are folded onto their delays one after the other (neighbouring tiles share delays), a lane per delay
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int i = 0; i < 4; ++i) tile[wave][n][4 * q + i][l15] = acc[n][i];
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int tc = 4 * cg + n;
            if (on && tc < nT && lane < nd) {
                int base = (16 * tc - 16 * tr - 15) % L;
                if (base < 0) base += L;
                int delta = base + lane;
                delta %= L;
                float sum = 0.f;
                bool any = false;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int t = 16 * tr + i;
                    int t2 = t + delta;
                    if (t2 >= L) t2 -= L;
                    const int col = t2 - 16 * tc;
                    const bool hit = t < L && col >= 0 && col < 16;
                    const float x = tile[wave][n][i][hit ? col : 0];
                    if (hit) { sum += x; any = true; }
                }
                if (any) rw[wave][delta] += sum;
            }
            // the next tile's lanes add to delays this tile's lanes wrote: keep the wave's LDS traffic in program order
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    rs[tid] = ((rw[0][tid] + rw[1][tid]) + rw[2][tid]) + rw[3][tid];
    __syncthreads();
    if (tid < L) {
        float acc = 0.f;
        int n = tid;                                        // (delta + tau) mod L, delta rising
        for (int delta = 0; delta < L; ++delta) {
            acc = fmaf(rs[delta], hs[n], acc);
            n = n + 1 == L ? 0 : n + 1;
        }
        const float mv = acc * (1.0f / (float)D);
        ms[tid] = mv;
        P.m[b * L + tid] = mv;
    }
    if (P.train) return;
    __syncthreads();
    if (wave == 0) fea_topk_wave(ms, L, P.topk, lane, P.idx + b * P.topk);
}

// grid 1, 1024 lanes (training mode)
__global__ void __launch_bounds__(1024) fea_select_kernel(const FeaP P) {
    __shared__ float part[4][256];
    __shared__ float g[256];
    const int tid = threadIdx.x, tau = tid & 255, slice = tid >> 8, L = P.L, B = P.B;
    float acc = 0.f;
    if (tau < L) {
#pragma unroll 4
        for (int b = slice; b < B; b += 4) acc += P.m[(long)b * L + tau];
    }
    part[slice][tau] = acc;
    __syncthreads();
    if (tid < 256) g[tid] = (((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]) * (1.0f / (float)B);
    __syncthreads();
    if (tid < 64) fea_topk_wave(g, L, P.topk, tid, P.idx);
}

// grid (B, ceil(L D / 4 / 256)), 256 lanes.  FWD: src = V, dst = out, shifts +idx, p computed here; else src = dOut, dst = dV,
// shifts -idx, p read.
template <bool FWD>
__global__ void __launch_bounds__(256) fea_shift_kernel(const FeaP P) {
    __shared__ float ps[32];
    __shared__ int sh[32];
    const int tid = threadIdx.x, L = P.L, D = P.D, d4 = D >> 2, k = P.topk;
    const long b = blockIdx.x;
    const int* idx = P.idx + (P.train ? 0 : b * k);
    if (tid < 64) {
        const bool in = tid < k;
        const int ix = in ? min(max(idx[tid], 0), L - 1) : 0;
        float pv;
        if (FWD) {
            const float mv = in ? P.m[b * L + ix] : -INFINITY;
            float mx = mv;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            const float e = in ? expf(mv - mx) : 0.f;
            float sum = e;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
            pv = e / sum;
            if (in && blockIdx.y == 0) P.p[b * k + tid] = pv;
        } else {
            pv = in ? P.p[b * k + tid] : 0.f;
        }
        if (in) {
            ps[tid] = pv;
            sh[tid] = FWD ? ix : (ix == 0 ? 0 : L - ix);
        }
    }
    __syncthreads();
    const int e = blockIdx.y * 256 + tid;
    if (e >= L * d4) return;
    const int t = e / d4, j = (e - t * d4) << 2;
    const float* src = (FWD ? P.v : P.dout) + b * L * D + j;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < k; ++i) {
        int t2 = t + sh[i];
        if (t2 >= L) t2 -= L;
        acc += ps[i] * ld4(src + (long)t2 * D);
    }
    st4((FWD ? P.out : P.dv) + (b * L + t) * D + j, acc);
}

// grid B, 256 lanes
__global__ void __launch_bounds__(256) fea_dp_kernel(const FeaP P) {
    __shared__ float ps[32], dps[32], dms[32], wsum[4], hs[256];
    __shared__ int sh[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = P.L, D = P.D, d4 = D >> 2, k = P.topk;
    const long b = blockIdx.x;
    const int* idx = P.idx + (P.train ? 0 : b * k);
    if (tid < k) { ps[tid] = P.p[b * k + tid]; sh[tid] = min(max(idx[tid], 0), L - 1); }
    hs[tid] = tid < L ? P.h[tid] : 0.f;
    __syncthreads();
    const float* go = P.dout + b * L * D;
    const float* vb = P.v + b * L * D;
    for (int i = 0; i < k; ++i) {
        const int s = sh[i];
        float acc = 0.f;
        for (int e = tid; e < L * d4; e += 256) {
            const int t = e / d4, j = (e - t * d4) << 2;
            int t2 = t + s;
            if (t2 >= L) t2 -= L;
            const f32x4 g = ld4(go + (long)t * D + j), x = ld4(vb + (long)t2 * D + j);
            acc += ((g[0] * x[0] + g[1] * x[1]) + g[2] * x[2]) + g[3] * x[3];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) wsum[wave] = acc;
        __syncthreads();
        if (tid == 0) dps[i] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        __syncthreads();
    }
    if (tid < k) {
        float dot = 0.f;
        for (int j = 0; j < k; ++j) dot += ps[j] * dps[j];
        dms[tid] = ps[tid] * (dps[tid] - dot);
    }
    __syncthreads();
    if (tid < L) {
        float acc = 0.f;
        for (int i = 0; i < k; ++i) {
            int n = tid + sh[i];
            if (n >= L) n -= L;
            acc = fmaf(dms[i], hs[n], acc);
        }
        P.cv[b * L + tid] = acc;
    }
}

// grid (B, 2), 256 lanes: y = 0 writes dQ from K, y = 1 dK from Q
__global__ void __launch_bounds__(256) fea_dqk_kernel(const FeaP P) {
    __shared__ float cs[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q = lane >> 4;
    const int L = P.L, D = P.D, nT = (L + 15) >> 4, nC = (D + 63) >> 6;
    const long b = blockIdx.x;
    const bool forq = blockIdx.y == 0;
    const float* X = (forq ? P.k : P.q) + b * L * D;
    float* Y = (forq ? P.dq : P.dk) + b * L * D;
    cs[tid] = tid < L ? P.cv[b * L + tid] : 0.f;
    __syncthreads();
    const float scale = 1.0f / (float)D;
    for (int it = wave; it < nT * nC; it += 4) {            // no barrier in this loop
        const int tr = it / nC, cb = it - tr * nC;
        const int row = 16 * tr + l15, col = 64 * cb + 4 * l15;
        const bool cin = col < D;
        f32x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < L; k0 += 4) {
            const int kk = k0 + q;
            // dQ: A[t][t'] = cv[(t' - t) mod L]; dK: A[t'][t] = cv[(t' - t) mod L]
            const bool ain = row < L && kk < L;
            int n = ain ? (forq ? kk - row : row - kk) : 0;
            if (n < 0) n += L;
            const float a = ain ? cs[n] : 0.f;
            const f32x4 bf = cin && kk < L ? ld4(X + (long)kk * D + col) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = fea_mfma(a, bf[c], acc[c]);
        }
        // register i of tile c: row 16 tr + 4 q + i, channel 64 cb + 4 l15 + c
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = 16 * tr + 4 * q + i;
            if (t < L && cin) st4(Y + (long)t * D + col, f32x4{acc[0][i], acc[1][i], acc[2][i], acc[3][i]} * scale);
        }
    }
}
