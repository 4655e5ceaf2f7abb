// Linear recurrent unit layer of the LRURec sibling model (bsarec_lru_fwd / bsarec_lru_bwd, include/bsarec_hip.h).  Width d,
// x [B][L][d], m_t = (ids[b][t] != 0), complex diagonal lambda; all arithmetic is fp32:
//   lambda = exp(-exp(nu_log)) (cos(exp(theta_log)) + i sin(exp(theta_log))),  gamma = exp(gamma_log)
//   u_t = W_in x_t + b_in (first d entries real, last d imaginary);  v_t = m_t gamma u_t;  h_t = lambda h_{t-1} + v_t, h_{-1} = 0
//   y_t = W_out [Re h_t | Im h_t] + b_out
// and t descending, with g_t = W_out^T dy_t read as a complex d-vector:
//   a_t = g_t + conj(lambda) a_{t+1} (a_L = 0);  lhat = sum_{b, t >= 1} a_t conj(h_{t-1});  dgamma_log = sum Re(a_t conj(v_t))
//   du_t = m_t gamma a_t;  z = lhat conj(lambda);  dnu_log = -exp(nu_log) Re z;  dtheta_log = exp(theta_log) Im z
//
// Every product (u, y, g, dx, the two weight gradients with the bias gradients as their column sums) goes through the GEMM core
// as the GRU's do (dense_nt / dense_nn / dense_tn / slab_sum).  What is new here is the scan.  Every activation is [B][L][2d], real
// half then imaginary half, in the rows' own order: no row map, no transposition.
//
// Scan kernels.  A workgroup of 256 threads owns SEQS sequences; a thread owns 4 adjacent channels (two 16-byte loads per step)
// of one of NC time chunks of one sequence.  CQ = d / 4, NC = min(16, 256 / CQ), SEQS = 256 / (CQ NC) are functions of d alone
// (d = 64: 16 chunks, 1 sequence; d = 256: 4 chunks, 1 sequence; d = 4: 16 chunks, 16 sequences); a chunk is
// CL = ceil(L / NC) steps, NU = ceil(L / CL) chunks hold steps.
//   pass 1   the chunk's recurrence from 0: its end value.  The loads do not depend on the recurrence.
//   carry    end values through LDS, one barrier; the thread of chunk c folds the ends of the chunks in front of it, in order,
//            with lambda^CL (CL - 1 multiplications by lambda, in order): carry_c = lambda^CL carry_{c-1} + end_{c-1}
//   pass 2   the chunk's recurrence again from its carry, with the same instructions: h (or du) is stored.  The second read
//            of the operands comes from cache.
// Run from an exact carry pass 2 IS the serial recurrence, so the carry's rounding is the only departure from a serial scan.
// The backward mirrors it with conj(lambda) from the right; the last chunk may be short, but its carry is 0, so the power that
// multiplies a carry is always lambda^CL.  It keeps lhat and dgamma_log per thread (12 accumulators), adds them in the
// workgroup in (sequence, chunk) order and writes ONE row per workgroup; lru_param_grad_kernel adds the rows in one fixed order
// and applies z and the two exp factors.
// A masked step takes v = 0 and du = 0 by selection, not by a product: h stays 0 exactly until a sequence's first item whatever
// x holds under the padding, an all-padded row gives h = 0, y = b_out bit for bit and dx = 0.  A thread reads and writes its own
// sequence alone and the chunking depends on (L, d) alone: a sequence's bits do not depend on B or on its place in the batch.
// No atomics, no allocation, no host synchronisation; LDS is static (8 KB forward, 20 KB backward).
#pragma once
#include "gru.h"

#define LRU_THREADS 256
#define LRU_MAX_CHUNKS 16

struct LruGeom { int cq, nc, seqs; };
__host__ __device__ __forceinline__ LruGeom lru_geom(int d) {
    LruGeom g;
    g.cq = d / 4;
    g.nc = LRU_THREADS / g.cq < LRU_MAX_CHUNKS ? LRU_THREADS / g.cq : LRU_MAX_CHUNKS;
    g.seqs = LRU_THREADS / (g.cq * g.nc);
    return g;
}

// lam = Re lambda [d] | Im lambda [d] | exp(gamma_log) [d], from the head of the flat weight array.  libm's expf / sincosf: an
// error of the angle is multiplied by t.
__global__ void __launch_bounds__(256) lru_lambda_kernel(const float* __restrict__ w, float* __restrict__ lam, int d) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const float mag = expf(-expf(w[j]));
    float sn, cs;
    sincosf(expf(w[d + j]), &sn, &cs);
    lam[j] = mag * cs;
    lam[d + j] = mag * sn;
    lam[2 * d + j] = expf(w[2 * d + j]);
}

// h <- (lr + i li) h + v, per channel of the quad; conj: h <- (lr - i li) h + v.  Explicit fmaf: both passes round alike.
template <bool CONJ>
__device__ __forceinline__ void lru_step(f32x4& hr, f32x4& hi, const f32x4& lr, const f32x4& li, const f32x4& vr, const f32x4& vi) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float s = CONJ ? -li[k] : li[k];
        const float nr = fmaf(lr[k], hr[k], fmaf(-s, hi[k], vr[k]));
        const float ni = fmaf(lr[k], hi[k], fmaf(s, hr[k], vi[k]));
        hr[k] = nr; hi[k] = ni;
    }
}

// (pr + i pi) = (lr + i s li)^n by n - 1 multiplications, n >= 1
template <bool CONJ>
__device__ __forceinline__ void lru_power(const f32x4& lr, const f32x4& li, int n, f32x4& pr, f32x4& pi) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    pr = lr; pi = CONJ ? -li : li;
    for (int k = 1; k < n; ++k) {
        f32x4 r = zero, i = zero;
        lru_step<CONJ>(pr, pi, lr, li, r, i);
    }
}

struct LruThread { int q, c, sl, b, t0, t1, nu, cl; bool live; };
__device__ __forceinline__ LruThread lru_thread(int B, int L, int d) {
    const LruGeom g = lru_geom(d);
    const int per = g.cq * g.nc, tid = threadIdx.x;
    LruThread T;
    T.sl = tid / per;
    const int r = tid - T.sl * per;
    T.c = r / g.cq;
    T.q = r - T.c * g.cq;
    T.b = blockIdx.x * g.seqs + T.sl;
    T.cl = (L + g.nc - 1) / g.nc;
    T.nu = (L + T.cl - 1) / T.cl;
    T.t0 = T.c * T.cl;
    T.t1 = T.t0 + T.cl < L ? T.t0 + T.cl : L;
    T.live = T.sl < g.seqs && T.b < B && T.t0 < L;
    return T;
}

struct LruFwdP {
    float* V;               // [B][L][2d]: u on entry; v on exit when save_v
    float* H;               // [B][L][2d]
    const int64_t* ids;     // [B][L] or null
    const float* lam;       // [3d]
    int B, L, d, save_v;
};

// grid ceil(B / SEQS)
__global__ void __launch_bounds__(LRU_THREADS) lru_scan_fwd_kernel(const LruFwdP P) {
    __shared__ __attribute__((aligned(16))) float ends[LRU_THREADS * 8];
    const int d = P.d, L = P.L;
    const LruThread T = lru_thread(P.B, L, d);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 lr = zero, li = zero, gm = zero, hr = zero, hi = zero;
    const long row0 = T.live ? (long)T.b * L : 0;
    float* v0 = P.V + row0 * (2 * d) + 4 * T.q;
    if (T.live) {
        lr = ld4(P.lam + 4 * T.q); li = ld4(P.lam + d + 4 * T.q); gm = ld4(P.lam + 2 * d + 4 * T.q);
#pragma unroll 4
        for (int t = T.t0; t < T.t1; ++t) {
            const bool m = !P.ids || P.ids[row0 + t] != 0;
            const float* p = v0 + (long)t * (2 * d);
            const f32x4 vr = m ? gm * ld4(p) : zero, vi = m ? gm * ld4(p + d) : zero;
            lru_step<false>(hr, hi, lr, li, vr, vi);
        }
    }
    st4(ends + threadIdx.x * 8, hr); st4(ends + threadIdx.x * 8 + 4, hi);
    __syncthreads();
    if (!T.live) return;
    hr = zero; hi = zero;
    if (T.c > 0) {
        f32x4 pr, pi;
        lru_power<false>(lr, li, T.cl, pr, pi);
        const float* e = ends + (threadIdx.x - T.c * (d / 4)) * 8;            // chunk 0 of this sequence and quad
        for (int j = 0; j < T.c; ++j, e += (d / 4) * 8) lru_step<false>(hr, hi, pr, pi, ld4(e), ld4(e + 4));
    }
    float* h0 = P.H + row0 * (2 * d) + 4 * T.q;
#pragma unroll 4
    for (int t = T.t0; t < T.t1; ++t) {
        const bool m = !P.ids || P.ids[row0 + t] != 0;
        float* p = v0 + (long)t * (2 * d);
        const f32x4 vr = m ? gm * ld4(p) : zero, vi = m ? gm * ld4(p + d) : zero;
        if (P.save_v) { st4(p, vr); st4(p + d, vi); }
        lru_step<false>(hr, hi, lr, li, vr, vi);
        float* h = h0 + (long)t * (2 * d);
        st4(h, hr); st4(h + d, hi);
    }
}

struct LruBwdP {
    float* G;               // [B][L][2d]: g on entry, du on exit
    const float* V;         // [B][L][2d]
    const float* H;         // [B][L][2d]
    const int64_t* ids;
    const float* lam;
    float* part;            // [grid][3d]: lhat real | lhat imaginary | dgamma_log, of the workgroup's sequences
    int B, L, d;
};

// grid ceil(B / SEQS)
__global__ void __launch_bounds__(LRU_THREADS) lru_scan_bwd_kernel(const LruBwdP P) {
    __shared__ __attribute__((aligned(16))) float ends[LRU_THREADS * 8];
    __shared__ __attribute__((aligned(16))) float accs[LRU_THREADS * 12];
    const int d = P.d, L = P.L;
    const LruThread T = lru_thread(P.B, L, d);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 lr = zero, li = zero, gm = zero, ar = zero, ai = zero;
    const long row0 = T.live ? (long)T.b * L : 0;
    float* g0 = P.G + row0 * (2 * d) + 4 * T.q;
    if (T.live) {
        lr = ld4(P.lam + 4 * T.q); li = ld4(P.lam + d + 4 * T.q); gm = ld4(P.lam + 2 * d + 4 * T.q);
#pragma unroll 4
        for (int t = T.t1 - 1; t >= T.t0; --t) {
            const float* p = g0 + (long)t * (2 * d);
            lru_step<true>(ar, ai, lr, li, ld4(p), ld4(p + d));
        }
    }
    st4(ends + threadIdx.x * 8, ar); st4(ends + threadIdx.x * 8 + 4, ai);
    __syncthreads();
    f32x4 sr = zero, si = zero, sg = zero;            // lhat and dgamma_log of this thread's steps
    if (T.live) {
        ar = zero; ai = zero;
        if (T.c < T.nu - 1) {
            f32x4 pr, pi;
            lru_power<true>(lr, li, T.cl, pr, pi);
            const float* e = ends + (threadIdx.x + (T.nu - 1 - T.c) * (d / 4)) * 8;      // the last chunk that holds steps
            for (int j = T.nu - 1; j > T.c; --j, e -= (d / 4) * 8) lru_step<false>(ar, ai, pr, pi, ld4(e), ld4(e + 4));
        }
        const float* v0 = P.V + row0 * (2 * d) + 4 * T.q;
        const float* h0 = P.H + row0 * (2 * d) + 4 * T.q;
#pragma unroll 2
        for (int t = T.t1 - 1; t >= T.t0; --t) {
            const bool m = !P.ids || P.ids[row0 + t] != 0;
            float* p = g0 + (long)t * (2 * d);
            const float* v = v0 + (long)t * (2 * d);
            const float* hp = h0 + (long)(t > 0 ? t - 1 : 0) * (2 * d);
            const f32x4 vr = ld4(v), vi = ld4(v + d);
            const f32x4 hr = t > 0 ? ld4(hp) : zero, hi = t > 0 ? ld4(hp + d) : zero;
            lru_step<true>(ar, ai, lr, li, ld4(p), ld4(p + d));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sr[k] = fmaf(ar[k], hr[k], fmaf(ai[k], hi[k], sr[k]));
                si[k] = fmaf(ai[k], hr[k], fmaf(-ar[k], hi[k], si[k]));
                sg[k] = fmaf(ar[k], vr[k], fmaf(ai[k], vi[k], sg[k]));
            }
            st4(p, m ? gm * ar : zero); st4(p + d, m ? gm * ai : zero);
        }
    }
    float* a = accs + threadIdx.x * 12;
    st4(a, sr); st4(a + 4, si); st4(a + 8, sg);
    __syncthreads();
    if (T.sl == 0 && T.c == 0) {                      // one thread per quad adds (sequence, chunk) in order
        const LruGeom g = lru_geom(d);
        sr = zero; si = zero; sg = zero;
        for (int s = 0; s < g.seqs && blockIdx.x * g.seqs + s < P.B; ++s)
            for (int c = 0; c < T.nu; ++c) {
                const float* x = accs + ((s * g.nc + c) * g.cq + T.q) * 12;
                sr += ld4(x); si += ld4(x + 4); sg += ld4(x + 8);
            }
        float* o = P.part + (long)blockIdx.x * (3 * d) + 4 * T.q;
        st4(o, sr); st4(o + d, si); st4(o + 2 * d, sg);
    }
}

// grid d / 4: workgroup q adds the nrows rows of part for its quad -- thread i rows i, i + 256, ... in order, then the 256
// threads pairwise through LDS -- and writes dnu_log, dtheta_log and dgamma_log of its 4 channels
__global__ void __launch_bounds__(256) lru_param_grad_kernel(const float* __restrict__ part, int nrows, const float* __restrict__ w,
                                                              const float* __restrict__ lam, int d, float* __restrict__ dw) {
    __shared__ __attribute__((aligned(16))) float red[256 * 12];
    const int q = blockIdx.x, tid = threadIdx.x;
    f32x4 sr = {0.f, 0.f, 0.f, 0.f}, si = sr, sg = sr;
    for (int r = tid; r < nrows; r += 256) {
        const float* x = part + (long)r * (3 * d) + 4 * q;
        sr += ld4(x); si += ld4(x + d); sg += ld4(x + 2 * d);
    }
    float* a = red + tid * 12;
    st4(a, sr); st4(a + 4, si); st4(a + 8, sg);
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if (tid < n) {
            const float* o = a + n * 12;
            sr += ld4(o); si += ld4(o + 4); sg += ld4(o + 8);
            st4(a, sr); st4(a + 4, si); st4(a + 8, sg);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const f32x4 lr = ld4(lam + 4 * q), li = ld4(lam + d + 4 * q), nu = ld4(w + 4 * q), th = ld4(w + d + 4 * q);
        f32x4 dnu, dth;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float zr = fmaf(sr[k], lr[k], si[k] * li[k]), zi = fmaf(si[k], lr[k], -(sr[k] * li[k]));
            dnu[k] = -expf(nu[k]) * zr;
            dth[k] = expf(th[k]) * zi;
        }
        st4(dw + 4 * q, dnu); st4(dw + d + 4 * q, dth); st4(dw + 2 * d + 4 * q, sg);
    }
}
