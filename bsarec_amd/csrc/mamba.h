// Selective state-space layer of the Mamba4Rec sibling model (bsarec_mamba_fwd / bsarec_mamba_bwd, include/bsarec_hip.h).
// Width d, d_inner = E d (written di), state N, convolution K, rank R, x [B][L][d], m_t = (ids[b][t] != 0); all fp32:
//   [xs_t | z_t] = W_in x_t;  c_t[j] = b_conv[j] + sum_{k<K} w_conv[j][k] m_s xs_s[j], s = t-K+1+k >= 0;  u_t = silu(c_t)
//   [delta_t | B_t | C_t] = W_x u_t;  Delta_t = softplus(W_dt delta_t + b_dt);  A = -exp(A_log)
//   m_t: h_t[j][n] = exp(Delta_t[j] A[j][n]) h_{t-1}[j][n] + Delta_t[j] B_t[n] u_t[j];  else h_t = h_{t-1};  h_{-1} = 0
//   s_t[j] = sum_n C_t[n] h_t[j][n] + D[j] u_t[j];  y_t = m_t ? s_t silu(z_t) : 0;  out_t = W_out y_t
// and t descending, with dy_t = W_out^T dout_t, ds_t = m_t ? dy_t silu(z_t) : 0 and a_t = exp(Delta_t A):
//   e_t = ds_t C_t + (m_{t+1} ? a_{t+1} : 1) e_{t+1};  dC_t[n] = sum_j ds_t h_t;  and at an item's position only
//   dDelta_t[j] = sum_n e_t (h_{t-1} a_t A + B_t u_t);  dB_t[n] = sum_j e_t Delta_t u_t;  du_t[j] = sum_n e_t Delta_t B_t + ds_t D
//   dA_log[j][n] = A sum_t e_t h_{t-1} a_t Delta_t;  dD[j] = sum_t ds_t u_t;  dz_t = dy_t s_t silu'(z_t)
//
// Every product (in_proj, the two halves of x_proj, dt_proj, out_proj, their dX and split-K dW, dt_proj.bias's gradient as the
// column sums of its dW product) goes through the GEMM core as the GRU's do (dense_nt / dense_nn / dense_tn / slab_sum).  dt_proj is a
// product too although its K = R may be 4: by count it is T di R multiply-adds, 1 / (2 d / R) of in_proj's, and a per-row dot
// inside the scan would repeat it in each of the N lanes of a channel.  New here are the convolution and the scan.
//
// mamba_conv_fwd_kernel / mamba_conv_bwd_kernel: element-wise in the channel.  The forward's thread owns 4 channels of one row and
// reads K rows of xs.  The backward's workgroup owns a run of rows and a thread a channel: dc = (du_scan + du_proj) silu'(c),
// dxs of its rows (dc of the K - 1 rows behind a row is formed again, not exchanged) and d conv1d.weight / d conv1d.bias of its
// rows in registers, written as ONE partial row per workgroup; mamba_rows_sum_kernel adds the partial rows in one fixed order.
//
// mamba_scan_fwd_kernel: a thread owns one (b, j, n) and time is serial in it; the N states of a channel sit in adjacent lanes,
// so s_t is a butterfly over N lanes.  A workgroup of 256 threads owns 256 / N channels of one sequence (a "slice").  The
// loads of a step do not depend on the recurrence and are issued four steps ahead, and neither does exp(Delta A) (libm expf:
// the state multiplies it L times); the dependent chain of a step is one fmaf.  In training it stores h after every
// MAMBA_CK-th step only (checkpoints), never [B][L][di][N].
// mamba_scan_bwd_kernel: walks the checkpoints from the right; a chunk's MAMBA_CK states and decays are formed again from its
// checkpoint with the forward's step function and stay in registers, with every operand of the chunk loaded in one batch in
// front of them, then e runs down the chunk.  dDelta and du are butterflies over the N lanes of a channel; dB and dC are sums
// over channels: a butterfly over the channels of a wave, then the four waves through LDS in wave order (two barriers per
// chunk), written as one partial row per slice that mamba_bc_sum_kernel adds in slice order.  dA_log and dD stay in registers
// over t (and over the sequences b, b + G, ... of a workgroup, G = min(B, 1024)) and are written as one row per sequence group;
// mamba_rows_sum_kernel adds them.
// Padding is a selection, never a product: h stays 0 exactly until the first item whatever x holds under the padding, y = 0 at
// a padded position, and ds, dz, du, dDelta, dB, dC are exact zeros there.  A thread reads and writes its own sequence alone and
// the chunking depends on L alone: a sequence's bits do not depend on B or on its place in the batch.
// No atomics, no allocation, no host synchronisation; LDS is static (<= 8 KB scan backward, 4 KB row sum).
#pragma once
#include "gru.h"

#define MAMBA_THREADS 256
#define MAMBA_CK 8

// log(1 + e^x) without overflow: above 20 the sum rounds to x in fp32
__device__ __forceinline__ float mamba_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float mamba_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// One step of a state: the decay a = exp(dt A) (returned) and h <- m ? a h + (dt Bn) u : h.  The forward and the backward's
// recomputation both go through here.
__device__ __forceinline__ float mamba_step(float& h, bool m, float dt, float A, float Bn, float u) {
    const float a = expf(dt * A);
    const float hn = fmaf(a, h, (dt * Bn) * u);
    h = m ? hn : h;
    return a;
}

// the sum of v over the lanes that differ in the bits [lo, hi) of the lane index, in every one of them
__device__ __forceinline__ float mamba_butterfly(float v, int lo, int hi) {
    for (int o = lo; o < hi; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- convolution -----------------------------------------------------------------------------------------------------------
struct MambaConvP {
    const float* XZ;        // [T][2 di]: xs | z
    const int64_t* ids;     // [B][L] or null
    const float* W;         // conv1d.weight [di][K], conv1d.bias [di] right behind it
    float* C;               // [T][di] pre-activation, or null (forward, train = 0)
    float* U;               // [T][di] forward: silu(c)
    const float* DU1;       // [T][di] backward: du of the scan
    const float* DU2;       // [T][di] backward: du of x_proj
    float* DXZ;             // [T][2 di] backward: dxs into the first di columns
    float* part;            // [workgroups][di K + di] backward
    long T;
    int L, di, K, rows;     // rows: the rows of a backward workgroup
};

// grid ceil(T di / 4 / 256)
__global__ void __launch_bounds__(256) mamba_conv_fwd_kernel(const MambaConvP P) {
    const int di = P.di, q4 = di / 4, K = P.K, L = P.L;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.T * q4) return;
    const long row = i / q4;
    const int j = (int)(i - row * q4) * 4, t = (int)(row % L);
    f32x4 acc = ld4(P.W + (long)di * K + j);
    for (int k = 0; k < K; ++k) {
        const int back = K - 1 - k;
        if (back > t || (P.ids && P.ids[row - back] == 0)) continue;
        const f32x4 xs = ld4(P.XZ + (row - back) * (2 * di) + j);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = fmaf(P.W[(j + c) * K + k], xs[c], acc[c]);
    }
    if (P.C) st4(P.C + row * di + j, acc);
    f32x4 u;
#pragma unroll
    for (int c = 0; c < 4; ++c) u[c] = acc[c] * mamba_sigmoid(acc[c]);
    st4(P.U + row * di + j, u);
}

// d silu(c) / dc times the incoming gradient
__device__ __forceinline__ float mamba_dc(const MambaConvP& P, long row, int j) {
    const float c = P.C[row * P.di + j], g = P.DU1[row * P.di + j] + P.DU2[row * P.di + j], sg = mamba_sigmoid(c);
    return g * (sg * fmaf(c, 1.0f - sg, 1.0f));
}

// grid ceil(T / rows)
__global__ void __launch_bounds__(256) mamba_conv_bwd_kernel(const MambaConvP P) {
    const int di = P.di, K = P.K, L = P.L;
    const long r0 = (long)blockIdx.x * P.rows, r1 = r0 + P.rows < P.T ? r0 + P.rows : P.T;
    float* part = P.part + (long)blockIdx.x * (di * K + di);
    for (int j = threadIdx.x; j < di; j += 256) {
        float w[4] = {0.f, 0.f, 0.f, 0.f}, dw[4] = {0.f, 0.f, 0.f, 0.f}, db = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < K) w[k] = P.W[j * K + k];
        for (long row = r0; row < r1; ++row) {
            const int t = (int)(row % L);
            const float dc = mamba_dc(P, row, j);
            db += dc;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int back = K - 1 - k;
                if (k < K && back <= t && (!P.ids || P.ids[row - back] != 0)) dw[k] = fmaf(dc, P.XZ[(row - back) * (2 * di) + j], dw[k]);
            }
            float dxs = 0.f;                              // xs of this row feeds c of the rows t .. t + K - 1 of its sequence
            if (!P.ids || P.ids[row] != 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ahead = K - 1 - k;
                    if (k < K && t + ahead < L) dxs = fmaf(w[k], ahead ? mamba_dc(P, row + ahead, j) : dc, dxs);
                }
            }
            P.DXZ[row * (2 * di) + j] = dxs;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < K) part[j * K + k] = dw[k];
        part[di * K + j] = db;
    }
}

// grid width / 4: workgroup q adds the nrows rows of part for its 4 columns -- thread i rows i, i + 256, ... in order, then the
// 256 threads pairwise through LDS
__global__ void __launch_bounds__(256) mamba_rows_sum_kernel(const float* __restrict__ part, int nrows, long width, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float red[256 * 4];
    const int q = blockIdx.x, tid = threadIdx.x;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int r = tid; r < nrows; r += 256) s += ld4(part + (long)r * width + 4 * q);
    float* a = red + tid * 4;
    st4(a, s);
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if (tid < n) { s += ld4(a + n * 4); st4(a, s); }
        __syncthreads();
    }
    if (tid == 0) st4(out + 4 * q, s);
}

// out[row][col0 + c] = the nslice partial rows [slice][T][w] added in slice order; grid ceil(T w / 4 / 256)
__global__ void __launch_bounds__(256) mamba_bc_sum_kernel(const float* __restrict__ part, int nslice, long T, int w, float* __restrict__ out,
                                                            int ldo, int col0) {
    const int w4 = w / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * w4) return;
    const long row = i / w4;
    const int c = (int)(i - row * w4) * 4;
    f32x4 s = ld4(part + row * w + c);
    for (int k = 1; k < nslice; ++k) s += ld4(part + ((long)k * T + row) * w + c);
    st4(out + row * ldo + col0 + c, s);
}

// ---- scan ------------------------------------------------------------------------------------------------------------------
struct MambaScanP {
    const float* XZ;        // [T][2 di]: z in the last di columns
    const float* U;         // [T][di]
    const float* DTR;       // [T][di] dt_proj's output, before softplus
    const float* BC;        // [T][2 N]: B_t | C_t
    const float* Alog;      // [di][N]
    const float* D;         // [di]
    const int64_t* ids;     // [B][L] or null
    float* Y;               // [T][di] forward
    float* S;               // [T][di] s_t: written by the training forward (null otherwise), read by the backward
    float* HCK;             // [B][nck][di][N] h after step c MAMBA_CK - 1, c = 1 .. nck: as S
    const float* DY;        // [T][di] backward
    float* DU;              // [T][di] backward
    float* DDT;             // [T][di] backward: the gradient of DTR
    float* DXZ;             // [T][2 di] backward: dz into the last di columns
    float* BCP;             // [slices][T][2 N] backward: dB_t | dC_t of a slice's channels
    float* ADP;             // [G][di N + di] backward: dA_log | dD of a sequence group
    int B, L, di, nck;
};

// What a thread reads per step.  The loads of a step depend on no earlier step, so both kernels issue them PF (forward) or a
// whole chunk (backward) of steps ahead of their use: a step then costs its arithmetic, not a round trip to memory.
struct MambaIn { float u, dt, Bn, Cn, z; bool m; };
template <int N>
__device__ __forceinline__ MambaIn mamba_load(const MambaScanP& P, long row, int jc, int n) {
    MambaIn v;
    v.m = !P.ids || P.ids[row] != 0;
    v.u = P.U[row * P.di + jc];
    v.dt = P.DTR[row * P.di + jc];
    v.Bn = P.BC[row * (2 * N) + n];
    v.Cn = P.BC[row * (2 * N) + N + n];
    v.z = P.XZ[row * (2 * P.di) + P.di + jc];
    return v;
}

// grid (B, ceil(di / (256 / N)))
template <int N>
__global__ void __launch_bounds__(MAMBA_THREADS) mamba_scan_fwd_kernel(const MambaScanP P) {
    constexpr int CH = MAMBA_THREADS / N, PF = 4;
    const int di = P.di, L = P.L, n = threadIdx.x % N, j = blockIdx.y * CH + threadIdx.x / N;
    const bool live = j < di;
    const int jc = live ? j : di - 1;                   // a dead lane repeats the last channel and stores nothing
    const int b = blockIdx.x;
    const long row0 = (long)b * L;
    const float A = -expf(P.Alog[jc * N + n]), Dj = P.D[jc];
    float h = 0.f;
    MambaIn cur[PF], nxt[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) cur[k] = mamba_load<N>(P, row0 + (k < L ? k : L - 1), jc, n);
    for (int tb = 0; tb < L; tb += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) nxt[k] = mamba_load<N>(P, row0 + (tb + PF + k < L ? tb + PF + k : L - 1), jc, n);
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = tb + k;
            if (t < L) {                                // the same for every thread
                const long row = row0 + t;
                const MambaIn& v = cur[k];
                mamba_step(h, v.m, mamba_softplus(v.dt), A, v.Bn, v.u);
                const float p = mamba_butterfly(v.Cn * h, 1, N);
                if (live && n == 0) {
                    const float s = fmaf(Dj, v.u, p);
                    P.Y[row * di + j] = v.m ? s * (v.z * mamba_sigmoid(v.z)) : 0.f;
                    if (P.S) P.S[row * di + j] = s;
                }
                if (P.HCK && live && (t + 1) % MAMBA_CK == 0 && t + 1 < L)
                    P.HCK[(((long)b * P.nck + (t + 1) / MAMBA_CK - 1) * di + j) * N + n] = h;
            }
        }
#pragma unroll
        for (int k = 0; k < PF; ++k) cur[k] = nxt[k];
    }
}

// grid (G, ceil(di / (256 / N))): workgroup (g, slice) runs the sequences g, g + G, ... one after the other
template <int N>
__global__ void __launch_bounds__(MAMBA_THREADS) mamba_scan_bwd_kernel(const MambaScanP P) {
    constexpr int CH = MAMBA_THREADS / N, CK = MAMBA_CK;
    __shared__ float red[CK][MAMBA_THREADS / 64][2 * N];
    const int di = P.di, L = P.L, tid = threadIdx.x, n = tid % N, j = blockIdx.y * CH + tid / N;
    const int lane = tid & 63, wave = tid >> 6;
    const bool live = j < di;
    const int jc = live ? j : di - 1;
    const long T = (long)P.B * L;
    const float A = -expf(P.Alog[jc * N + n]), Dj = P.D[jc];
    const int nchunk = (L + CK - 1) / CK;
    float accA = 0.f, accD = 0.f;
    for (int b = blockIdx.x; b < P.B; b += gridDim.x) {
        const long row0 = (long)b * L;
        float e = 0.f;                                  // (m_{t+1} ? a_{t+1} : 1) e_{t+1}
        for (int c = nchunk - 1; c >= 0; --c) {
            const int t0 = c * CK;
            const float h0 = c > 0 ? P.HCK[(((long)b * P.nck + c - 1) * di + jc) * N + n] : 0.f;
            MambaIn in[CK];
            float dy[CK], sv[CK], hs[CK], as[CK];
#pragma unroll
            for (int k = 0; k < CK; ++k) {              // every load of the chunk, before any of its arithmetic
                const long row = row0 + (t0 + k < L ? t0 + k : L - 1);
                in[k] = mamba_load<N>(P, row, jc, n);
                dy[k] = P.DY[row * di + jc];
                sv[k] = P.S[row * di + jc];
            }
            float h = h0;
#pragma unroll
            for (int k = 0; k < CK; ++k) {
                float a = 1.f;
                if (t0 + k < L) {
                    in[k].dt = mamba_softplus(in[k].dt);
                    a = mamba_step(h, in[k].m, in[k].dt, A, in[k].Bn, in[k].u);
                }
                hs[k] = h; as[k] = a;
            }
#pragma unroll
            for (int k = CK - 1; k >= 0; --k) {
                float cB = 0.f, cC = 0.f;
                if (t0 + k < L) {                       // the same for every thread
                    const long row = row0 + t0 + k;
                    float du = 0.f, ddt = 0.f, dz = 0.f;
                    if (in[k].m) {                      // the same for every thread
                        const float u = in[k].u, dt = in[k].dt, Bn = in[k].Bn, Cn = in[k].Cn, z = in[k].z;
                        const float sg = mamba_sigmoid(z), ds = dy[k] * (z * sg);
                        const float hprev = k > 0 ? hs[k > 0 ? k - 1 : 0] : h0, a = as[k];
                        const float et = fmaf(ds, Cn, e), da = et * hprev;
                        cC = live ? ds * hs[k] : 0.f;
                        cB = live ? et * (dt * u) : 0.f;
                        accA = fmaf(da * a, dt, accA);
                        accD = fmaf(ds, u, accD);
                        // d softplus(x) / dx = sigmoid(x) = 1 - exp(-softplus(x)), formed without the cancellation
                        ddt = mamba_butterfly(fmaf(da, a * A, et * (Bn * u)), 1, N) * -expm1f(-dt);
                        du = fmaf(ds, Dj, mamba_butterfly(et * (dt * Bn), 1, N));
                        dz = dy[k] * sv[k] * (sg * fmaf(z, 1.0f - sg, 1.0f));
                        e = a * et;
                    }
                    if (live && n == 0) {
                        P.DU[row * di + j] = du;
                        P.DDT[row * di + j] = ddt;
                        P.DXZ[row * (2 * di) + di + j] = dz;
                    }
                }
                cB = mamba_butterfly(cB, N, 64);
                cC = mamba_butterfly(cC, N, 64);
                if (lane < N) { red[k][wave][lane] = cB; red[k][wave][N + lane] = cC; }
            }
            __syncthreads();
            for (int i = tid; i < CK * 2 * N; i += MAMBA_THREADS) {
                const int k = i / (2 * N), col = i - k * (2 * N);
                if (t0 + k < L)
                    P.BCP[((long)blockIdx.y * T + row0 + t0 + k) * (2 * N) + col] =
                        ((red[k][0][col] + red[k][1][col]) + red[k][2][col]) + red[k][3][col];
            }
            __syncthreads();
        }
    }
    if (live) {
        float* o = P.ADP + (long)blockIdx.x * ((long)di * N + di);
        o[j * N + n] = accA * A;
        if (n == 0) o[di * N + j] = accD;
    }
}
