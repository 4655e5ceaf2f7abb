// The parts of a GRU4Rec training step around the GRU stack (bsarec_gru4rec_loss_grad / bsarec_gru4rec_train_step,
// include/bsarec_hip.h): the dropped-out embedding lookup, the B-row BPR head and the whole item-table gradient.  All fp32; rows
// are float4 lanes as in kernels.h (ROW_THREADS lanes, LPR lanes per row, d <= 256, d % 4 == 0).
//   gru4rec_embed_kernel      x[b, t, :] = E[ids[b, t]] * m, m = the Philox keep-mask of dropout site 0 times 1 / (1 - p); the element
//                             index of the stream is (b L + t) d + c, i.e. oracle/bsarec_oracle.py::dropout_keep(B L d, p, seed,
//                             step, 0).  Id 0 is an ordinary row (nn.Embedding without padding_idx).  Its lanes also clear the
//                             fixed-point accumulator of the item-table gradient, so that a step does not depend on what the
//                             workspace holds on entry.
//   gru4rec_bpr_kernel        per row b, with s = the stack's [B, d] output: diff = s . E[a_b] - s . E[n_b], loss_b = -log(sig(diff) +
//                             1e-10), c_b = d(mean loss) / d(diff) = -sig (1 - sig) / (sig + 1e-10) / B, ds_b = c_b (E[a_b] - E[n_b]).
//   gru4rec_item_grad_kernel  dE in one pass over T + 2 B rows: row r < T adds dx[r, :] * m to row ids[r] (the mask regenerated, not
//                             stored), row T + b adds c_b s_b to row a_b, row T + B + b adds -(c_b s_b) to row n_b.
//   gru4rec_flush_kernel      accumulator -> EVERY float of d_item_emb (zero where no row was touched, LookupAcc.dense_zero) and, in
//                             one closing block, the mean loss in a fixed order and -- in a training step -- Adam's t (tick_body).
//
// The gradient rows are summed as the BSARec lookup path sums them (kernels.h: lookup_fix, embed_scatter_block, lookup_flush):
// 64-bit fixed point in 2^-40 units, an addend clamped to |x| <= 2^22, so |sum| < 2^22 after the clamp is exact -- the same range as
// the BSARec lookup path.  Duplicates of a chunk are folded in LDS and one global integer row add goes out per distinct id and
// chunk; integer adds commute, so dE has the same bits on every run whatever order tokens and chunks arrive in.  x and -x round to
// opposite integers: a row with a_b == n_b contributes exactly zero.  embed_scatter_block itself skips id 0 (BSARec's padding_idx)
// and reads 32-bit ids of one source; the block below is its body without the skip, over three row sources.
//
// ids, answers and negatives inside [0, V) are the caller's contract; a value outside is never dereferenced (its x row is zero, its
// gradient row is dropped).
#pragma once
#include "kernels.h"

struct Gru4RecEmbedP {
    const float* E; const int64_t* ids; float* x;
    long T; int d, V;
    DropP drop;
    unsigned long long* acc; long acc_n2;       // the accumulator as pairs of 64-bit words, cleared here
};

template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) gru4rec_embed_kernel(const Gru4RecEmbedP P) {
    constexpr int RPP = ROW_THREADS / LPR;
    const int lr = threadIdx.x / LPR, lc = (threadIdx.x % LPR) << 2;
    const DropSeed sd = drop_seed(P.drop);
    if (lc < P.d) {
        for (long r = (long)blockIdx.x * RPP + lr; r < P.T; r += (long)gridDim.x * RPP) {
            const long id = P.ids[r];
            const long e = r * P.d + lc;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (id >= 0 && id < P.V) v = ld4(P.E + id * P.d + lc) * drop_mult4(P.drop, sd, (uint64_t)e >> 2);
            st4(P.x + e, v);
        }
    }
    ulonglong2* a = reinterpret_cast<ulonglong2*>(P.acc);
    for (long i = (long)blockIdx.x * ROW_THREADS + threadIdx.x; i < P.acc_n2; i += (long)gridDim.x * ROW_THREADS)
        a[i] = make_ulonglong2(0ull, 0ull);
}

// sig(x) and 1 - sig(x), each formed from e^{-|x|} <= 1: 0 or 1 exactly for large |x| (e^{-|x|} underflows to 0), never NaN for a
// finite or infinite x, and no cancellation in 1 - sig
__device__ __forceinline__ void gru4rec_sigmoid(float x, float& sg, float& one_minus) {
    const float e = expf(-fabsf(x));
    const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
    sg = x >= 0.f ? big : small;
    one_minus = x >= 0.f ? small : big;
}

struct Gru4RecBprP {
    const float* s; const float* E; const int64_t* ans; const int64_t* neg;
    int B, d, V;
    float* ds; float* c; float* loss_rows;
};

template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) gru4rec_bpr_kernel(const Gru4RecBprP P) {
    constexpr int RPP = ROW_THREADS / LPR;
    const int lr = threadIdx.x / LPR, lc = (threadIdx.x % LPR) << 2;
    const int b = blockIdx.x * RPP + lr;
    const bool rowok = b < P.B, ok = rowok && lc < P.d;
    long ia = 0, in = 0;
    if (rowok) { ia = P.ans[b]; in = P.neg[b]; }
    const bool idok = ia >= 0 && ia < P.V && in >= 0 && in < P.V;
    f32x4 sv = {0.f, 0.f, 0.f, 0.f}, ea = sv, en = sv;
    if (ok && idok) {
        sv = ld4(P.s + (long)b * P.d + lc);
        ea = ld4(P.E + ia * P.d + lc);
        en = ld4(P.E + in * P.d + lc);
    }
    // every lane of the wave takes part in the row sums (rows behind B and columns behind d add zeros)
    const f32x4 pa = sv * ea, pn = sv * en;
    const float da = group_sum<LPR>((pa.x + pa.y) + (pa.z + pa.w)), dn = group_sum<LPR>((pn.x + pn.y) + (pn.z + pn.w));
    float sg, om;
    gru4rec_sigmoid(da - dn, sg, om);
    const float cb = -(sg * om) / (sg + 1e-10f) / (float)P.B;
    if (ok) st4(P.ds + (long)b * P.d + lc, cb * (ea - en));
    if (rowok && lc == 0) {
        P.c[b] = cb;
        P.loss_rows[b] = -logf(sg + 1e-10f);
    }
}

struct Gru4RecGradP {
    const float* dx; const int64_t* ids;                 // [T, d], [T]
    const float* s; const float* c;                      // [B, d], [B]
    const int64_t* ans; const int64_t* neg;              // [B]
    long T; int B, d, V;
    DropP drop;
    unsigned long long* dA;                              // [V][d] fixed point, zero on entry
};

// grid ceil((T + 2 B) / CHUNK), CHUNK = SCATTER_FLOATS / (4 LPR) rows per block
template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) gru4rec_item_grad_kernel(const Gru4RecGradP P) {
    constexpr int RPP = ROW_THREADS / LPR, W = LPR * 4, CHUNK = SCATTER_FLOATS / W, NP = CHUNK / RPP;
    __shared__ __attribute__((aligned(16))) unsigned long long acc[SCATTER_FLOATS];       // [CHUNK][W]
    __shared__ __attribute__((aligned(16))) int sid[CHUNK];
    __shared__ int lead[CHUNK];
    const int lr = threadIdx.x / LPR, lc = (threadIdx.x % LPR) << 2, d = P.d;
    const bool colok = lc < d;
    const long T = P.T, R = T + 2L * P.B;
    const long r0 = (long)blockIdx.x * CHUNK;
    const int n = (int)(R - r0 < CHUNK ? R - r0 : CHUNK);
    const DropSeed sd = drop_seed(P.drop);
    for (int i = threadIdx.x; i < CHUNK; i += ROW_THREADS) {
        long id = -1;                                    // no row: never equal to an id, never added
        if (i < n) {
            const long r = r0 + i;
            id = r < T ? P.ids[r] : (r < T + P.B ? P.ans[r - T] : P.neg[r - T - P.B]);
            if (id < 0 || id >= P.V) id = -1;
        }
        sid[i] = (int)id;
    }
    for (int i = threadIdx.x; i < SCATTER_FLOATS; i += ROW_THREADS) acc[i] = 0ull;
    __syncthreads();
    f32x4 g[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int j = lr + p * RPP;
        g[p] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (colok && j < n && sid[j] >= 0) {
            const long r = r0 + j;
            if (r < T) {
                const long e = r * d + lc;
                g[p] = ld4(P.dx + e) * drop_mult4(P.drop, sd, (uint64_t)e >> 2);
            } else {
                const bool isneg = r >= T + P.B;
                const long b = r - T - (isneg ? P.B : 0);
                const f32x4 v = P.c[b] * ld4(P.s + b * d + lc);
                g[p] = isneg ? -v : v;
            }
        }
    }
    for (int j = threadIdx.x; j < CHUNK; j += ROW_THREADS) {          // first occurrence of sid[j] in the chunk: its leader
        const int id = sid[j];
        int l = j;
        for (int i = CHUNK - 4; i >= 0; i -= 4) {
            const int4 q = *reinterpret_cast<const int4*>(sid + i);
            if (q.w == id && i + 3 < l) l = i + 3;
            if (q.z == id && i + 2 < l) l = i + 2;
            if (q.y == id && i + 1 < l) l = i + 1;
            if (q.x == id && i < l) l = i;
        }
        lead[j] = l;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int j = lr + p * RPP;
        if (colok && j < n && sid[j] >= 0) {
            unsigned long long* a = acc + lead[j] * W + lc;
            atomicAdd(a + 0, lookup_fix(g[p].x)); atomicAdd(a + 1, lookup_fix(g[p].y));
            atomicAdd(a + 2, lookup_fix(g[p].z)); atomicAdd(a + 3, lookup_fix(g[p].w));
        }
    }
    __syncthreads();
    // one leader row per wave instruction, lane = column: a global 64-bit add covers contiguous bytes of one row
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr int PW = CHUNK / (ROW_THREADS / 64);       // rows owned by one wave (<= 16)
    const int j0 = wv * PW, myj = j0 + lane;
    const bool is_leader = lane < PW && myj < n && sid[myj] >= 0 && lead[myj] == myj;
    unsigned long long todo = __ballot(is_leader);
    while (todo) {
        const int j = j0 + __builtin_ctzll(todo);
        todo &= todo - 1;
        const long row = (long)sid[j] * d;
        for (int c0 = 0; c0 < d; c0 += 64)
            if (c0 + lane < d) atomicAdd(P.dA + row + c0 + lane, acc[j * W + c0 + lane]);
    }
}

// blocks [0, la.nblocks): accumulator -> la.dst, every float written; the block behind them closes the step
__global__ void __launch_bounds__(ROW_THREADS) gru4rec_flush_kernel(const LookupAcc la, const TickP tk) {
    __shared__ float red[ROW_THREADS];
    if ((int)blockIdx.x >= la.nblocks) { tick_body(tk, red); return; }
    lookup_flush(la, (long)blockIdx.x * ROW_THREADS + threadIdx.x, (long)la.nblocks * ROW_THREADS);
}
