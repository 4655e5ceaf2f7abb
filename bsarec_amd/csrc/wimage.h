// Fragment-ordered fp32 image of the Linear weights.
//
// The fp32 block kernels hold a weight operand as MFMA B fragments: per 32-wide tile of output columns and per 8-deep
// k-block, lane (j, h) -- j = column inside the tile, h = lane half -- holds the four values k = 8 kb + 4 h + {0..3} of
// column j.  Read from the row-major master that is one 16-byte piece out of 32 different rows per wave instruction
// ("rows x weights", load_w) or four dword loads a row apart ("x . W", load_wT).  The image stores every weight a second
// and third time in exactly that order, so that the fragment of one (tile, k-block) is 1 KB contiguous, 16 bytes per lane
// in lane order: one fully coalesced load per wave and k-block, the same values in the same registers.
//
//   F image of W[N][K] (forward, B[k][n] = W[n][k]):  W[n][k] at wimage_off(n, k, K)
//   T image of W[N][K] (backward, B[r][c] = W[r][c]): W[r][c] at wimage_off(c, r, N)      (= the F image of W^T)
//
// Both are N K floats.  Per layer the six weights follow each other in the order wq, wk, wv, wo, w1, w2 (WIMAGE_* below),
// first all F images, then all T images.
#pragma once
#include <hip/hip_runtime.h>

// col: the fragment's column (the lane's j + 32 x tile), k: position along the reduction, kdim: its length (% 8 == 0)
__host__ __device__ inline long wimage_off(int col, int k, int kdim) {
    const int tile = col >> 5, kb = k >> 3, lane = (col & 31) + 32 * ((k >> 2) & 1);
    return ((long)(tile * (kdim >> 3) + kb) * 64 + lane) * 4 + (k & 3);
}

// element offsets of the six weights inside one orientation of a layer's image, d = hidden size (wq, wk, wv, wo: d x d;
// w1: 4d x d; w2: d x 4d), and the size of a layer's image (both orientations)
enum { WIMAGE_WQ, WIMAGE_WK, WIMAGE_WV, WIMAGE_WO, WIMAGE_W1, WIMAGE_W2, WIMAGE_NW };
__host__ __device__ inline long wimage_weight_off(int which, long d) { return (which < 4 ? which : 4 * which - 12) * d * d; }
__host__ __device__ inline long wimage_layer_floats(long d) { return 2 * 12 * d * d; }

#ifdef __HIPCC__
// W[n][k] of a weight [wn][wk] into both images (f, t: the weight's F and T image)
__device__ __forceinline__ void wimage_store(float* __restrict__ f, float* __restrict__ t, int n, int k, int wn, int wk, float v) {
    f[wimage_off(n, k, wk)] = v;
    t[wimage_off(k, n, wn)] = v;
}
#endif
