// The user half of the personalised Caser step (bsarec_caser_user_loss_grad / bsarec_caser_user_train_step,
// include/bsarec_hip.h): with z1 = relu(fc1(Dropout(z))) [B, d] of caser_step.h, a user table P [U, d] and users [B],
//   x2 = [ z1 | P[users] ] [B, 2 d];   s = relu(fc2(x2)),  fc2 = Linear(2 d, d)
// fc2 runs on the launches of fc1 (caser_fc_fwd_launch / caser_fc_bwd_launch with F' = 2 d and no mask): this file holds only
// what stands around them.  All fp32; rows are float4 lanes as in kernels.h (ROW_THREADS lanes, LPR lanes per row, d <= 256,
// d % 4 == 0, so a float4 never straddles the halves of x2).
//   caser_user_concat_kernel  x2[b, 0:d] = z1[b], x2[b, d:2d] = P[users[b]] (zeros for an id outside [0, U)).  Its lanes also
//                             clear the fixed-point accumulator of the user-table gradient, as pair_embed_kernel clears the
//                             item table's (acc_clear): a step does not depend on what the workspace holds on entry.
//   caser_user_grad_kernel    with dx2 [B, 2 d] of fc2's dz launch: blocks [0, scatter_blocks) run fix_scatter_block over the B
//                             rows -- row b adds dx2[b, d:2d] to row users[b] of the [U][d] accumulator, duplicates folded in
//                             LDS -- and the blocks behind them copy dx2[b, 0:d] into the contiguous dz1 [B, d] that fc1's
//                             backward reads as its ds.
// The accumulator goes into EVERY float of d_user_emb through pair_flush_kernel on a grid of la.nblocks (lookup_flush with
// dense_zero: zero where no row of the batch names the user), so without the closing block: the item flush behind it closes the
// step.
// The scatter is the one of kernels.h: 64-bit fixed point in 2^-40 units, exact while |sum| < 2^22, integer adds, so d_user_emb
// has the same bits on every run.  A user id outside [0, U) is never dereferenced and adds nothing (pair_row_id).
#pragma once
#include "pair_step.h"

struct CaserUserP {
    const float* z1;            // [B][d]
    const float* P;             // [U][d]
    const int64_t* users;       // [B]
    float* x2;                  // [B][2 d]
    const float* dx2;           // [B][2 d]
    float* dz1;                 // [B][d]
    int B, d, U;
    unsigned long long* acc;    // [U][d] fixed point: cleared by the concat, added to by the gradient
    long acc_n2;                // the accumulator as pairs of 64-bit words
    int scatter_blocks;         // the gradient launch: blocks in front that scatter
};

// grid min(ceil(B / RPP), 4096), RPP = ROW_THREADS / LPR rows per pass
template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) caser_user_concat_kernel(const CaserUserP P) {
    constexpr int RPP = ROW_THREADS / LPR;
    const int lr = threadIdx.x / LPR, lc = (threadIdx.x % LPR) << 2;
    if (lc < P.d) {
        for (long b = (long)blockIdx.x * RPP + lr; b < P.B; b += (long)gridDim.x * RPP) {
            const long u = P.users[b];
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (u >= 0 && u < P.U) v = ld4(P.P + u * P.d + lc);
            const long e = b * 2 * P.d + lc;
            st4(P.x2 + e, ld4(P.z1 + b * P.d + lc));
            st4(P.x2 + e + P.d, v);
        }
    }
    acc_clear(P.acc, P.acc_n2);
}

// grid scatter_blocks + ceil(B / RPP), scatter_blocks = ceil(B / CHUNK), CHUNK = SCATTER_FLOATS / (4 LPR) rows per block
template <int LPR>
__global__ void __launch_bounds__(ROW_THREADS) caser_user_grad_kernel(const CaserUserP P) {
    __shared__ __attribute__((aligned(16))) float lds[fix_scatter_lds_bytes(LPR) / 4];
    const int d = P.d;
    if ((int)blockIdx.x < P.scatter_blocks) {             // block-uniform
        fix_scatter_block<LPR>(P.B, d, P.acc, blockIdx.x, lds,
            [&](long r) { return pair_row_id(P.users[r], P.U); },
            [&](long r, int lc) { return ld4(P.dx2 + r * 2 * d + d + lc); });
        return;
    }
    constexpr int RPP = ROW_THREADS / LPR;
    const int lr = threadIdx.x / LPR, lc = (threadIdx.x % LPR) << 2;
    const long b = (long)(blockIdx.x - P.scatter_blocks) * RPP + lr;
    if (b < P.B && lc < d) st4(P.dz1 + b * d + lc, ld4(P.dx2 + b * 2 * d + lc));
}
