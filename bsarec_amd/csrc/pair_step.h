// What the pairwise training steps share around their encoders: the embedding lookup, the B-row BPR head and the whole
// item-table gradient.  Three steps launch these kernels (include/bsarec_hip.h): GRU4Rec (bsarec_gru4rec_*; the candidate heads
// of gru4rec_cand.h stand where the BPR rows do), Caser (bsarec_caser_*, caser_step.h) and the personalised Caser
// (bsarec_caser_user_*, caser_user.h).  Their host side is the PairStep shell of bsarec_hip.hip.  All fp32; rows are float4 lanes
// as in kernels.h (ROW_THREADS lanes, LPR lanes per row, d <= 256, d % 4 == 0).
//   pair_embed_kernel      x[b, t, :] = E[ids[b, t]] * m, m = the Philox keep-mask of dropout site 0 times 1 / (1 - p); the
//                          element index of the stream is (b L + t) d + c, i.e. oracle/bsarec_oracle.py::dropout_keep(B L d, p,
//                          seed, step, 0).  GRU4Rec drops its token rows out; both Casers pass no mask (m = 1: their dropout
//                          stands before fc1).  Id 0 is an ordinary row (nn.Embedding without padding_idx).  Its lanes also
//                          clear the fixed-point accumulator of the item-table gradient (acc_clear, kernels.h), so that a step
//                          does not depend on what the workspace holds on entry.
//   pair_bpr_kernel        per row b, with s = the encoder's [B, d] state: diff = s . E[a_b] - s . E[n_b], loss_b =
//                          -log(sig(diff) + 1e-10), c_b = d(mean loss) / d(diff) = -sig (1 - sig) / (sig + 1e-10) / B,
//                          ds_b = c_b (E[a_b] - E[n_b]).
//   pair_item_grad_kernel  dE in one pass over T + 2 B rows: row r < T adds dx[r, :] * m to row ids[r] (the mask regenerated,
//                          not stored), row T + b adds c_b s_b to row a_b, row T + B + b adds -(c_b s_b) to row n_b.
//   pair_flush_kernel      accumulator -> EVERY float of the table's gradient (zero where no row was touched,
//                          LookupAcc.dense_zero) and, in the block behind la.nblocks, the mean loss in a fixed order and -- in a
//                          training step -- Adam's t (tick_body).  A step launches that closing block exactly once, with its
//                          item-table flush; the user-table flush of the personalised Caser is this kernel on a grid of
//                          la.nblocks, so without it.
//
// The gradient rows are summed by the code that sums the BSARec lookup path (kernels.h: lookup_fix, fix_scatter_block,
// lookup_flush): 64-bit fixed point in 2^-40 units, an addend clamped to |x| <= 2^22, so |sum| < 2^22 after the clamp is exact.
// Duplicates of a chunk are folded in LDS and one global integer row add goes out per distinct id and chunk; integer adds commute,
// so dE has the same bits on every run whatever order tokens and chunks arrive in.  x and -x round to opposite integers: a row with
// a_b == n_b contributes exactly zero.  pair_item_grad_kernel only tells fix_scatter_block the id and the addend of row r, over
// its three row sources; BSARec's caller maps id 0 (its padding_idx) to "no row", this one maps ids outside [0, V) to it
// (pair_row_id).
//
// ids, answers and negatives inside [0, V) are the caller's contract; a value outside is never dereferenced (its x row is zero, its
// gradient row is dropped).
#pragma once
#include "kernels.h"

struct PairEmbedP {
    const float* E; const int64_t* ids; float* x;
    long T; int d, V;
    DropP drop;
    unsigned long long* acc; long acc_n2;       // the accumulator as pairs of 64-bit words, cleared here
};

template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) pair_embed_kernel(const PairEmbedP P) {
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
    acc_clear(P.acc, P.acc_n2);
}

// sig(x) and 1 - sig(x), each formed from e^{-|x|} <= 1: 0 or 1 exactly for large |x| (e^{-|x|} underflows to 0), never NaN for a
// finite or infinite x, and no cancellation in 1 - sig
__device__ __forceinline__ void pair_sigmoid(float x, float& sg, float& one_minus) {
    const float e = expf(-fabsf(x));
    const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);
    sg = x >= 0.f ? big : small;
    one_minus = x >= 0.f ? small : big;
}

struct PairBprP {
    const float* s; const float* E; const int64_t* ans; const int64_t* neg;
    int B, d, V;
    float* ds; float* c; float* loss_rows;
};

template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) pair_bpr_kernel(const PairBprP P) {
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
    pair_sigmoid(da - dn, sg, om);
    const float cb = -(sg * om) / (sg + 1e-10f) / (float)P.B;
    if (ok) st4(P.ds + (long)b * P.d + lc, cb * (ea - en));
    if (rowok && lc == 0) {
        P.c[b] = cb;
        P.loss_rows[b] = -logf(sg + 1e-10f);
    }
}

// The item-table gradient of a step under either head.  Rows [0, T) are the token rows; behind them stand the head's rows:
//   pair_item_grad_kernel                  2 B rows: T + b adds c[b] head_rows[b, :] to ans[b], T + B + b adds its negative to
//                                          neg[b]; head_rows = s [B, d]
//   g4c_item_grad_kernel (gru4rec_cand.h)  C rows: T + j adds head_rows[j, :] to candidate j; head_rows = dEc [C, d], c is not read
struct PairGradP {
    const float* dx; const int64_t* ids;                 // [T, d], [T]
    const float* head_rows; const float* c;
    const int64_t* ans; const int64_t* neg;              // [B]
    long T; int B, C, d, V;
    DropP drop;
    unsigned long long* dA;                              // [V][d] fixed point, zero on entry
};

// the scatter's id of an item: an id outside [0, V) is no row
__device__ __forceinline__ int pair_row_id(long id, int V) { return id >= 0 && id < V ? (int)id : -1; }
// token row r < T of either kernel: dx[r, lc .. lc + 3] times the regenerated dropout multiplier, into ids[r]
__device__ __forceinline__ f32x4 pair_token_row(const PairGradP& P, const DropSeed& sd, long r, int lc) {
    const long e = r * P.d + lc;
    return ld4(P.dx + e) * drop_mult4(P.drop, sd, (uint64_t)e >> 2);
}

// grid ceil((T + 2 B) / CHUNK), CHUNK = SCATTER_FLOATS / (4 LPR) rows per block
template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) pair_item_grad_kernel(const PairGradP P) {
    __shared__ __attribute__((aligned(16))) float lds[fix_scatter_lds_bytes(LPR) / 4];
    const long T = P.T, B = P.B;
    const DropSeed sd = drop_seed(P.drop);
    fix_scatter_block<LPR>(T + 2 * B, P.d, P.dA, blockIdx.x, lds,
        [&](long r) { return pair_row_id(r < T ? P.ids[r] : (r < T + B ? P.ans[r - T] : P.neg[r - T - B]), P.V); },
        [&](long r, int lc) {
            if (r < T) return pair_token_row(P, sd, r, lc);
            const bool isneg = r >= T + B;
            const long b = r - T - (isneg ? B : 0);
            const f32x4 v = P.c[b] * ld4(P.head_rows + b * P.d + lc);
            return isneg ? -v : v;
        });
}

// blocks [0, la.nblocks): accumulator -> la.dst, every float written; a block behind them closes the step.  Grid la.nblocks + 1:
// the item table's flush; grid la.nblocks: a flush alone, tk is not read.
__global__ void __launch_bounds__(ROW_THREADS) pair_flush_kernel(const LookupAcc la, const TickP tk) {
    __shared__ float red[ROW_THREADS];
    if ((int)blockIdx.x >= la.nblocks) { tick_body(tk, red); return; }
    lookup_flush(la, (long)blockIdx.x * ROW_THREADS + threadIdx.x, (long)la.nblocks * ROW_THREADS);
}
