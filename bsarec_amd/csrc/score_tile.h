// The one score tile of the catalogue kernels (full_rank.h, answer_rank.h, ce_head.h): 32 RB rows of h against the 32 items of
// a wave through v_mfma_f32_32x32x2_f32.  Per element the fp32 MFMA computes acc = 0, then acc = fmaf(h[k], e[k], acc) for
// k = 0 .. d-1 (one rounding per product, k ascending): the chain of fr_dot bit for bit, whichever kernel forms the score.
//   score_stage   rows of h -> LDS, row stride d + 4 floats
//   score_items   a wave's 32 item rows as a wave-uniform pointer and this lane's offset
//   score_tile    <RB, ROWS_IN_LANE>: the scores.  The MFMA takes its two operands either way round, which decides what a lane
//                 holds of a 32 x 32 block:
//                   ROWS_IN_LANE  (A = items, B = h):  lane (l31, half) holds row l31 and the 16 items rho(r) + 4 half
//                   !ROWS_IN_LANE (A = h, B = items):  lane (l31, half) holds item l31 and the 16 rows rho(r) + 4 half
// d % 4 == 0, d <= 256; E 16-byte aligned; ROW_THREADS lanes.  sh is read and written as float4: a kernel declares its dynamic
// LDS __attribute__((aligned(16))), or static LDS of an odd size in front of it turns every ds_read_b128 into a misaligned one.
#pragma once
#include "kernels.h"

// rows [r0, r0 + rows) of h (any row stride ldh >= d) into sh[rows][d + 4]; zeros behind row B.  Whole float4s when the rows
// are 16-byte aligned (h is, so ldh % 4 == 0 decides for the workgroup), single floats otherwise.  With a row list, row r is
// row list[r] of h (ce_head.h: the cloze head's scattered tokens); entries at or behind B are never read.  The list is a
// workgroup-uniform choice made once, outside the copy loops: without one the loops are the ones they always were.
template <bool LIST>
__device__ __forceinline__ void score_stage_rows(const float* __restrict__ h, long ldh, int B, int d, int r0, int rows, float* sh,
                                                 const int32_t* __restrict__ list) {
    const int dp = d + 4;
    if ((ldh & 3) == 0) {
        const int dq = d >> 2;
        for (int x = threadIdx.x; x < rows * dq; x += ROW_THREADS) {
            const int i = x / dq, c = (x - i * dq) << 2;
            f32x4 v = {0, 0, 0, 0};
            if (r0 + i < B) v = ld4(h + (long)(LIST ? list[r0 + i] : r0 + i) * ldh + c);
            st4(&sh[i * dp + c], v);
        }
    } else {
        for (int x = threadIdx.x; x < rows * d; x += ROW_THREADS) {
            const int i = x / d, c = x - i * d;
            sh[i * dp + c] = r0 + i < B ? h[(long)(LIST ? list[r0 + i] : r0 + i) * ldh + c] : 0.f;
        }
    }
}
__device__ __forceinline__ void score_stage(const float* __restrict__ h, long ldh, int B, int d, int r0, int rows, float* sh,
                                            const int32_t* __restrict__ list = nullptr) {
    if (list) score_stage_rows<true>(h, ldh, B, d, r0, rows, sh, list);
    else score_stage_rows<false>(h, ldh, B, d, r0, rows, sh, nullptr);
}
// A wave's 32 items i0 .. i0 + 31 (i0 wave-uniform) as a wave-uniform row pointer into E and this lane's offset from it in
// floats (item i0 + l31); an item behind V reads a row that exists.
__device__ __forceinline__ const float* score_items(const float* __restrict__ E, int V, int d, unsigned i0, unsigned& off) {
    off = i0 + (threadIdx.x & 31) < (unsigned)V ? (threadIdx.x & 31) * (unsigned)d : 0u;
    return E + (long)(i0 < (unsigned)V ? i0 : 0u) * d;
}
// The scores of RB row blocks (LDS rows 32 rb + l31 of sh) against the item of this lane (ebase + eoff, score_items).
template <int RB, bool ROWS_IN_LANE>
__device__ __forceinline__ void score_tile(const float* sh, const float* __restrict__ ebase, unsigned eoff, int d, f32x16 (&acc)[RB]) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, dp = d + 4;
    const float4* e4 = reinterpret_cast<const float4*>(ebase + eoff);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rb][r] = 0.f;
    for (int kc = 0; kc < d; kc += 4) {
        const float4 e = e4[kc >> 2];
        const float e0 = half ? e.y : e.x, e1 = half ? e.w : e.z;       // MFMA k-step: lanes 0..31 give k, lanes 32..63 k + 1
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const float4 a = *reinterpret_cast<const float4*>(&sh[(rb * 32 + l31) * dp + kc]);
            const float a0 = half ? a.y : a.x, a1 = half ? a.w : a.z;
            if (ROWS_IN_LANE) {
                acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(e0, a0, acc[rb], 0, 0, 0);
                acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(e1, a1, acc[rb], 0, 0, 0);
            } else {
                acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, e0, acc[rb], 0, 0, 0);
                acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, e1, acc[rb], 0, 0, 0);
            }
        }
    }
}
