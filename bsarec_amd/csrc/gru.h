// GRU stack of the GRU4Rec sibling model (bsarec_gru_fwd / bsarec_gru_bwd, include/bsarec_hip.h): N layers of torch's bias-free
// GRU cell in gate order (r, z, n), h_0 = 0, and an optional Linear on top.  All arithmetic is fp32.
//   a_t = W_ih x_t, b_t = W_hh h_{t-1}:  r = s(a_r + b_r), z = s(a_z + b_z), n = tanh(a_n + r b_n), h_t = n + z (h_{t-1} - n)
//
// Everything that is not serial in t goes through the GEMM core (gemm.h): the input projections A = X . W_ih^T of all L B rows, the
// output projection, and after the backward's serial loop dX = da . W_ih, dW_ih = da^T . X, dW_hh = db^T . H_prev, dW_out, db_out.
// The weight gradients are TN split-K products into slabs that gru_slab_sum_kernel adds in split order.
//
// Layout.  Inside the workspace every activation is TIME-MAJOR, [L][B][.]: the rows of one step of a tile of sequences are
// contiguous, and h_{t-1} of row (t, b) is the row B places earlier, so dW_hh = db[1..L-1]^T . Y[0..L-2] is ONE product over
// (L - 1) B rows of two shifted views (the h_{-1} = 0 terms drop out).  The interface tensors are [B][L][.]: EpiGru writes a
// product's rows through the row map, gru_swap_rows_kernel turns an operand.
//
// Sequence kernels.  A workgroup owns GRU_ROWS = 16 sequences for all L steps and talks to no other workgroup; H / 32 waves, wave
// w owns hidden units j = 32 w .. 32 w + 31 of ALL THREE gates, so the gate arithmetic of an element needs no exchange: register
// i of the 16 x 16 accumulators (gate g, column half c) of lane (l15, q) is row 4 q + i, unit 32 w + 16 c + l15 of r, z and n.
// 16-row tiles (v_mfma_f32_16x16x4_f32) instead of 32-row ones (32x32x2): the same MFMA rate, but half the MFMA chain, gates, loads
// and stores per step and twice the workgroups -- measured 0.666 -> 0.398 ms forward + backward at B = 256.
//   gru_seq_fwd_kernel  W_hh's rows of the wave's 96 columns stay in 3 H / 2 registers as B-operand fragments (k order inside
//                       a 16-deep block permuted, identically for h: lane (., q) takes k = 16 kb + 4 q + s in k-step (kb, s), so
//                       both operands are 16-byte reads);
//                       per step: a_t of the tile (global, issued before the products), b_t = h_{t-1} . W_hh^T from the h tile in
//                       LDS (two buffers, one barrier per step), the gates, h_t -> LDS, Y and, in training, r z n b_n -> S.
//   gru_seq_bwd_kernel  W_hh's COLUMNS 32 w .. + 31 stay in 3 H / 2 registers; t runs down, dh is carried in registers;
//                       per step: the element part (below) from S, Y[t - 1] and dY -- loaded one step ahead, while the previous
//                       step's products run --, da and db_n -> global, db = (da_r, da_z, db_n) -> LDS, then dh = g z + db . W_hh as
//                       independent accumulator chains (one per gate block of the k axis and column half) added in gate order.
//   g = dY_t + dh; dn = g (1 - z); dz = g (h_{t-1} - n); da_n = dn (1 - n^2); db_n = da_n r; dr = da_n b_n;
//   da_r = db_r = dr r (1 - r); da_z = db_z = dz z (1 - z)
// A tile's rows behind B hold zeros in every operand (a = 0 keeps h = 0: n = tanh(0) = 0, h = n + z (0 - n)) and are never stored.
// A row of an MFMA result depends on its own operand row alone: a sequence's bits do not depend on its batch or tile.
// No atomics, no allocation, no host synchronisation; LDS is static (<= 24.3 KB), so nothing needs raising before a capture.
#pragma once
#include "epilogues.h"

#define GRU_ROWS 16

// out = acc [+ bias[n]], split-K slab `split` at c_split; row m = p Q + q of the product is row q P + p of C (P = 0: row m)
struct EpiGru {
    float* C; long ldc, c_split;
    const float* bias;                 // null: none
    int P, Q;

    template <int BM, int BN, int NT = GEMM_THREADS>
    __device__ __forceinline__ void run(const float* Cs, const TileCtx& c) const {
        constexpr int LDC = BN + 4, CV = BN / 4;
        float* out = C + (long)c.split * c_split;
        for (int idx = threadIdx.x; idx < BM * CV; idx += NT) {
            const int r = idx / CV, lc = (idx % CV) << 2;
            const int m = c.m0 + r, n = c.n0 + lc;
            if (m >= c.M || n >= c.N) continue;
            f32x4 v = ld4(Cs + r * LDC + lc);
            if (bias) v += ld4(bias + n);
            const long row = P ? (long)(m % Q) * P + m / Q : (long)m;
            st4(out + row * ldc + n, v);
        }
    }
};

// dst [Q][P][4 W4] = src [P][Q][4 W4]
__global__ void __launch_bounds__(256) gru_swap_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, long P, long Q, int W4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P * Q * W4) return;
    const long row = i / W4, c = i - row * W4, p = row / Q, q = row - p * Q;
    st4(dst + ((q * P + p) * W4 + c) * 4, ld4(src + i * 4));
}

// out[4 i ..] = the nslab slabs of n4 float4 added in slab order
__global__ void __launch_bounds__(256) gru_slab_sum_kernel(const float* __restrict__ slab, int nslab, long n4, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 a = ld4(slab + 4 * i);
    for (int s = 1; s < nslab; ++s) a += ld4(slab + ((long)s * n4 + i) * 4);
    st4(out + 4 * i, a);
}

// The gates of a step are on its critical path beside 3 H / 2 MFMAs: v_exp_f32 and v_rcp_f32 (1 ulp each) instead of libm's
// expf / tanhf and an IEEE division, which cost about as many vector cycles per step as the MFMAs (forward launch 0.398 ->
// 0.278 ms at B = 256, L = 50, H = 64 with 32-row tiles).
// tanh as 1 - 2 / (1 + e^2x) is accurate to ~1e-7 ABSOLUTE (it cancels near 0), which is what h = n + z (h - n) needs; both
// saturate to their limits exactly (e^x = inf -> rcp = 0) and stay inside [0, 1] / [-1, 1].
__device__ __forceinline__ float gru_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float gru_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

struct GruFwdP {
    const float* A;         // [L][B][3H] input projections
    const float* Whh;       // [3H][H]
    float* Y;               // [L][B][H] the layer's output
    float* S;               // [L][B][4H] r | z | n | b_n for the backward, or null
    int B, L;
};

__device__ __forceinline__ f32x4 gru_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Element e < 8 of a lane (l15, q): tile row 4 q + (e & 3), hidden unit 32 wave + 16 (e >> 2) + l15 -- register e & 3 of the
// 16 x 16 accumulator of column half e >> 2.

// grid ceil(B / 16), 64 NH lanes; H = 32 NH
template <int NH>
__global__ void __launch_bounds__(64 * NH) gru_seq_fwd_kernel(const GruFwdP P) {
    constexpr int H = 32 * NH, LDH = H + 4;
    __shared__ __attribute__((aligned(16))) float hs[2][GRU_ROWS * LDH];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, q = lane >> 4;
    const int b0 = blockIdx.x * GRU_ROWS, j0 = wave * 32 + l15, B = P.B;

    float wf[3][2][H / 4];  // wf[g][c][4 kb + s] = W_hh[g H + j0 + 16 c][16 kb + 4 q + s]: the B operand of k-step (kb, s)
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int kb = 0; kb < H / 16; ++kb) {
                const f32x4 w = ld4(P.Whh + (long)(g * H + j0 + 16 * c) * H + kb * 16 + 4 * q);
#pragma unroll
                for (int s = 0; s < 4; ++s) wf[g][c][4 * kb + s] = w[s];
            }
    for (int x = tid; x < GRU_ROWS * LDH; x += 64 * NH) hs[0][x] = 0.f;
    float h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = 0.f;
    __syncthreads();

    for (int t = 0; t < P.L; ++t) {
        const float* hc = hs[t & 1];
        float* hn = hs[(t + 1) & 1];
        float a[3][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int b = b0 + 4 * q + (e & 3);
            const float* p = P.A + ((long)t * B + (b < B ? b : 0)) * (3 * H) + j0 + 16 * (e >> 2);
#pragma unroll
            for (int g = 0; g < 3; ++g) a[g][e] = b < B ? p[g * H] : 0.f;
        }
        f32x4 acc[3][2];
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[g][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < H / 16; ++kb) {
            const f32x4 af = ld4(hc + l15 * LDH + kb * 16 + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int g = 0; g < 3; ++g)
#pragma unroll
                    for (int c = 0; c < 2; ++c) acc[g][c] = gru_mfma(af[s], wf[g][c][4 * kb + s], acc[g][c]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = e >> 2, i = e & 3, row = 4 * q + i, b = b0 + row, j = j0 + 16 * c;
            const float rr = gru_sigmoid(a[0][e] + acc[0][c][i]), zz = gru_sigmoid(a[1][e] + acc[1][c][i]), bn = acc[2][c][i];
            const float nn = gru_tanh(a[2][e] + rr * bn);
            const float hv = nn + zz * (h[e] - nn);
            h[e] = hv;
            hn[row * LDH + j] = hv;
            if (b < B) {
                const long x = (long)t * B + b;
                P.Y[x * H + j] = hv;
                if (P.S) {
                    float* s = P.S + x * (4 * H) + j;
                    s[0] = rr; s[H] = zz; s[2 * H] = nn; s[3 * H] = bn;
                }
            }
        }
        lds_barrier();       // h_t complete before step t + 1 reads it; step t + 1 writes the OTHER buffer
    }
}

struct GruBwdP {
    const float* S;         // [L][B][4H]
    const float* Y;         // [L][B][H] the layer's output
    const float* Whh;       // [3H][H]
    const float* dY;        // [L][B][H]; dy_last: [B][H], the gradient at t = L - 1, zero elsewhere
    float* da;              // [L][B][3H]
    float* dbn;             // [L][B][H]
    int B, L, dy_last;
};

struct GruSaved { float r[8], z[8], n[8], bn[8], hp[8], dy[8]; };

template <int H>
__device__ __forceinline__ void gru_bwd_load(const GruBwdP& P, int t, int b0, int q, int j0, GruSaved& v) {
    const int B = P.B;
    const bool has_dy = !P.dy_last || t == P.L - 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int b = b0 + 4 * q + (e & 3), j = j0 + 16 * (e >> 2);
        const bool ok = b < B;
        const long x = (long)t * B + (ok ? b : 0);
        const float* s = P.S + x * (4 * H) + j;
        v.r[e] = ok ? s[0] : 0.f;
        v.z[e] = ok ? s[H] : 0.f;
        v.n[e] = ok ? s[2 * H] : 0.f;
        v.bn[e] = ok ? s[3 * H] : 0.f;
        v.hp[e] = ok && t > 0 ? P.Y[(x - B) * H + j] : 0.f;
        v.dy[e] = ok && has_dy ? P.dY[(P.dy_last ? (long)(ok ? b : 0) : x) * H + j] : 0.f;
    }
}

// grid ceil(B / 16), 64 NH lanes; H = 32 NH
template <int NH>
__global__ void __launch_bounds__(64 * NH) gru_seq_bwd_kernel(const GruBwdP P) {
    constexpr int H = 32 * NH, LDB = 3 * H + 4;
    __shared__ __attribute__((aligned(16))) float ds[GRU_ROWS * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l15 = lane & 15, q = lane >> 4;
    const int b0 = blockIdx.x * GRU_ROWS, j0 = wave * 32 + l15, B = P.B;

    float wb[3][2][H / 4];  // wb[g][c][4 kb + s] = W_hh[g H + 16 kb + 4 q + s][j0 + 16 c]: the B operand of k-step (g, kb, s)
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int ks = 0; ks < H / 4; ++ks) wb[g][c][ks] = P.Whh[(long)(g * H + 16 * (ks >> 2) + 4 * q + (ks & 3)) * H + j0 + 16 * c];
    float dh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) dh[e] = 0.f;

    GruSaved cur;
    gru_bwd_load<H>(P, P.L - 1, b0, q, j0, cur);
    GruSaved nxt = cur;
    for (int t = P.L - 1; t >= 0; --t) {
        float dhe[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int row = 4 * q + (e & 3), b = b0 + row, j = j0 + 16 * (e >> 2);
            const float rr = cur.r[e], zz = cur.z[e], nn = cur.n[e];
            const float g = cur.dy[e] + dh[e];
            const float dn = g * (1.0f - zz), dz = g * (cur.hp[e] - nn);
            dhe[e] = g * zz;
            const float dan = dn * (1.0f - nn * nn), dbn = dan * rr, dr = dan * cur.bn[e];
            const float dar = dr * rr * (1.0f - rr), daz = dz * zz * (1.0f - zz);
            float* d = ds + row * LDB + j;
            d[0] = dar; d[H] = daz; d[2 * H] = dbn;
            if (b < B) {
                const long x = (long)t * B + b;
                float* a = P.da + x * (3 * H) + j;
                a[0] = dar; a[H] = daz; a[2 * H] = dan;
                P.dbn[x * H + j] = dbn;
            }
        }
        lds_barrier();       // db of the tile complete
        if (t > 0) gru_bwd_load<H>(P, t - 1, b0, q, j0, nxt);        // lands while the products run
        f32x4 acc[3][2];
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[g][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < H / 16; ++kb) {
            f32x4 af[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) af[g] = ld4(ds + l15 * LDB + g * H + kb * 16 + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int g = 0; g < 3; ++g)
#pragma unroll
                    for (int c = 0; c < 2; ++c) acc[g][c] = gru_mfma(af[g][s], wb[g][c][4 * kb + s], acc[g][c]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) dh[e] = dhe[e] + ((acc[0][e >> 2][e & 3] + acc[1][e >> 2][e & 3]) + acc[2][e >> 2][e & 3]);
        lds_barrier();       // every wave has read db before step t - 1 overwrites it
        cur = nxt;
    }
}
