// The answer's exact rank in the full-catalogue order without a score matrix, a threshold, a candidate list, a select or a
// sort (bsarec_answer_rank / bsarec_answer_rank_range / bsarec_answer_score_range, include/bsarec_hip.h).  With a = answers[b]
// and the target (t, a), t = e(b, a) (or the caller's answer_score[b]), rank_out[b] = #{ j != a in the range : (e(b, j), j)
// stands before (t, a) } under topk_seen_kernel's total order: topk_key(e) > topk_key(t), or equal keys and GLOBAL j < a.
// Two launches on one stream, no workspace:
//   (a) answer_rank_row_kernel, one workgroup per row: t (the fmaf chain of fr_dot; +0 when a occurs in the CSR row) goes to
//       score_out, and rank_out[b] starts as the row's signed correction, so that (b) can count RAW scores only:
//         - [raw s(b, a) before the target]                          (a itself is in the range and (b) cannot skip it), and
//         for every DISTINCT seen item j != a of the range  + [(+0, j) before the target] - [(s(b, j), j) before the target].
//       A row without a valid target (its answer outside the range; with a given score: outside [0, 2^31)) gets -1 and NaN.
//       Distinct: the CSR row is taken in chunks of AR_CHUNK entries; a chunk's in-range ids go into an LDS table (rank_hash,
//       RANK_SLOTS slots, at most half full), which holds an id once however often the chunk repeats it.  For every chunk
//       after the first, the entries BEFORE the chunk are then streamed through the table and the ids they hit are marked
//       dead: an id counts in the chunk of its first occurrence only.  The correction walks the table's live slots.  A row
//       of n entries costs n table inserts, n rescored items at most, and sum over chunks c >= 1 of c * AR_CHUNK further
//       index loads and probes -- none for n <= 2048, 2048 for ML-1M's row of 2,314, n^2 / 4096 in general.
//   (b) answer_rank_count_kernel: the grid, LDS tile and score_tile call of full_rank_filter_kernel (128 rows of h, 32 items
//       per wave, the same scores bit for bit); the epilogue compares every accumulator element's key with its
//       row's threshold and adds into ONE INTEGER PER ACCUMULATOR ELEMENT per lane (64 VGPRs).  After the item loop the 32
//       lanes that hold a row are summed with shuffles, the four waves through LDS, and each row gets one atomicAdd per
//       workgroup.  (b) reads the target as (a) left it: answer_score[b], else score_out[b], else -- a caller that wants no
//       scores -- recomputed per tile row with the same code (ar_effective).
// Integer adds only: the result does not depend on the grid or on the order of the atomics.
// Column base: as in full_rank.h the item rows are [base, base + V); CSR entries and answers are GLOBAL ids, so the tie order
// between ranges is the global one and the ranks of a catalogue's contiguous ranges add up to the whole catalogue's.
#pragma once
#include "full_rank.h"

#define AR_CHUNK (RANK_SLOTS / 2)          // CSR entries per dedupe chunk: the table stays at most half full
#define AR_NONE_KEY 0xffffffffu            // threshold of a row without a target: above every key (NaN's is 0xffc00000)
#define AR_NONE_ANS 0x7fffffff             // ... and an answer no column reaches (base + V <= 2^31 - 1)

// (key, GLOBAL column j) before the target (tkey, a), j != a.
__device__ __forceinline__ bool ar_before(unsigned key, long j, unsigned tkey, long a) {
    return key > tkey || (key == tkey && j < a);
}
// Is the row's target defined?  Without a given score the answer must lie in the range; with one it only orders ties.
__device__ __forceinline__ bool ar_valid(long a, long base, int V, bool given) {
    return given ? (a >= 0 && a <= 0x7fffffffL) : fr_local(a, base, V) >= 0;
}
// e(b, a) for an answer inside the range, by ONE WAVE (all 64 lanes call it and get the same value): +0.0 when the GLOBAL id
// a occurs in CSR entries [j0, j1), else the fmaf chain.
__device__ __forceinline__ float ar_effective(const float* hs, const float* __restrict__ E, long base, int d, long a,
                                              const int64_t* __restrict__ indices, long j0, long j1) {
    const int lane = threadIdx.x & 63;
    bool seen = false;
    for (long j = j0; j < j1; j += 64) seen |= j + lane < j1 && indices[j + lane] == a;
    return __ballot(seen) ? 0.f : fr_dot(hs, E + (a - base) * d, d);
}

// (a).  SCORE_ONLY (bsarec_answer_score_range): score_out[b] = e(b, a) for the rows whose answer lies in the range, nothing else.
template <bool SCORE_ONLY>
__global__ void __launch_bounds__(ROW_THREADS)
answer_rank_row_kernel(const float* __restrict__ h, long ldh, const float* __restrict__ E, int V, long base, int d,
                       const int64_t* __restrict__ users, const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                       const int64_t* __restrict__ answers, const float* __restrict__ answer_score, int32_t* __restrict__ rank_out,
                       float* __restrict__ score_out) {
    __shared__ float hs[256];
    __shared__ int table[RANK_SLOTS];
    __shared__ unsigned dead[RANK_SLOTS / 32];
    __shared__ int wsum[ROW_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long a = answers[b];
    const bool given = !SCORE_ONLY && answer_score != nullptr;
    const long al = fr_local(a, base, V);                // the answer's local column, or -1
    if (!ar_valid(a, base, V, given)) {
        if (!SCORE_ONLY && tid == 0) { rank_out[b] = -1; if (score_out) score_out[b] = __builtin_nanf(""); }
        return;
    }
    for (int i = tid; i < d; i += ROW_THREADS) hs[i] = h[(long)b * ldh + i];
    __syncthreads();
    long j0 = 0, j1 = 0;
    if (indptr) { const long u = users[b]; j0 = indptr[u]; j1 = indptr[u + 1]; }
    const float t = given ? answer_score[b] : ar_effective(hs, E, base, d, a, indices, j0, j1);
    if (score_out && tid == 0) score_out[b] = t;
    if (SCORE_ONLY) return;
    const unsigned tkey = topk_key(t);
    int corr = 0;
    if (al >= 0 && tid == 0) corr = -(int)(topk_key(fr_dot(hs, E + al * d, d)) > tkey);
    for (long c0 = j0; c0 < j1; c0 += AR_CHUNK) {
        for (int i = tid; i < RANK_SLOTS; i += ROW_THREADS) table[i] = -1;
        for (int i = tid; i < RANK_SLOTS / 32; i += ROW_THREADS) dead[i] = 0u;
        __syncthreads();
        const long c1 = c0 + AR_CHUNK < j1 ? c0 + AR_CHUNK : j1;
        for (long j = c0 + tid; j < c1; j += ROW_THREADS) {
            const long it = fr_local(indices[j], base, V);
            if (it < 0 || it == al) continue;
            for (unsigned p = rank_hash((unsigned)it);; p = (p + 1) & (RANK_SLOTS - 1)) {
                const int old = atomicCAS(&table[p], -1, (int)it);
                if (old == -1 || old == (int)it) break;
            }
        }
        __syncthreads();
        if (c0 > j0) {                                   // ids that an earlier chunk has counted
            for (long j = j0 + tid; j < c0; j += ROW_THREADS) {
                const long it = fr_local(indices[j], base, V);
                if (it < 0) continue;
                for (unsigned p = rank_hash((unsigned)it);; p = (p + 1) & (RANK_SLOTS - 1)) {
                    const int v = table[p];
                    if (v == (int)it) { atomicOr(&dead[p >> 5], 1u << (p & 31)); break; }
                    if (v == -1) break;
                }
            }
            __syncthreads();
        }
        for (int p = tid; p < RANK_SLOTS; p += ROW_THREADS) {
            const int it = table[p];
            if (it < 0 || ((dead[p >> 5] >> (p & 31)) & 1u)) continue;
            const long g = base + it;
            corr += (int)ar_before(FR_KEY0, g, tkey, a) - (int)ar_before(topk_key(fr_dot(hs, E + (long)it * d, d)), g, tkey, a);
        }
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) corr += __shfl_xor(corr, off, 64);
    if (lane == 0) wsum[wave] = corr;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < ROW_THREADS / 64; ++w) s += wsum[w];
        rank_out[b] = s;
    }
}

// (b).  Dynamic LDS: FR_ROWS x (d + 4) floats of h.  tgt_s[i] = (threshold key, answer) of tile row i: element (i, item j)
// counts iff key >= tkey + (a <= j), which is ar_before (no carry: a real tkey is <= 0xffc00000).
__global__ void __launch_bounds__(ROW_THREADS)
answer_rank_count_kernel(const float* __restrict__ h, long ldh, const float* __restrict__ E, int B, int V, long base, int d,
                         const int64_t* __restrict__ users, const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                         const int64_t* __restrict__ answers, const float* __restrict__ answer_score,
                         const float* __restrict__ score_in, int32_t* rank_out) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    __shared__ uint2 tgt_s[FR_ROWS];
    __shared__ int cnt_s[FR_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, half = lane >> 5;
    const int r0 = blockIdx.x * FR_ROWS;
    const int dp = d + 4;
    score_stage(h, ldh, B, d, r0, FR_ROWS, sh);
    for (int i = tid; i < FR_ROWS; i += ROW_THREADS) cnt_s[i] = 0;
    __syncthreads();
    const bool given = answer_score != nullptr;
    const float* tsrc = given ? answer_score : score_in;
    if (tsrc) {
        for (int i = tid; i < FR_ROWS; i += ROW_THREADS) {
            const long a = r0 + i < B ? answers[r0 + i] : -1;
            tgt_s[i] = ar_valid(a, base, V, given) ? make_uint2(topk_key(tsrc[r0 + i]), (unsigned)a)
                                                   : make_uint2(AR_NONE_KEY, (unsigned)AR_NONE_ANS);
        }
    } else {
        constexpr int RW = FR_ROWS / (ROW_THREADS / 64);   // a wave takes RW tile rows, one after the other
        for (int i = wave * RW; i < (wave + 1) * RW; ++i) {
            const long a = r0 + i < B ? answers[r0 + i] : -1;
            uint2 tg = make_uint2(AR_NONE_KEY, (unsigned)AR_NONE_ANS);
            if (ar_valid(a, base, V, false)) {
                long j0 = 0, j1 = 0;
                if (indptr) { const long u = users[r0 + i]; j0 = indptr[u]; j1 = indptr[u + 1]; }
                tg = make_uint2(topk_key(ar_effective(&sh[i * dp], E, base, d, a, indices, j0, j1)), (unsigned)a);
            }
            if (lane == 0) tgt_s[i] = tg;
        }
    }
    __syncthreads();
    int cnt[4][16];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) cnt[rb][r] = 0;
    const int nblk = (V + FR_ITEMS - 1) / FR_ITEMS;
    for (int ib = blockIdx.y; ib < nblk; ib += gridDim.y) {
        const unsigned i0 = (unsigned)ib * FR_ITEMS + wave * 32;         // this wave's 32 items
        const int item = (int)i0 + l31;
        const bool iv = item < V;
        unsigned eoff;
        const float* eb = score_items(E, V, d, i0, eoff);
        f32x16 acc[4];
        score_tile<4, false>(sh, eb, eoff, d, acc);
        const int gj = (int)(base + item);
        if (iv) {                                        // ONE divergent region (the last block's tail), a branch-free body
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint2 tg = tgt_s[rb * 32 + rho(r) + 4 * half];   // row of the tile; column = item
                    const unsigned thr = tg.x + ((int)tg.y <= gj ? 1u : 0u);
                    cnt[rb][r] += (int)(topk_key(acc[rb][r]) >= thr);
                }
        }
    }
    // the 32 lanes of a half hold the same rows: sum them, then the waves through LDS, then one atomic per row
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int c = cnt[rb][r];
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
            if (l31 == 0 && c) atomicAdd(&cnt_s[rb * 32 + rho(r) + 4 * half], c);
        }
    __syncthreads();
    for (int i = tid; i < FR_ROWS; i += ROW_THREADS)
        if (cnt_s[i] && tgt_s[i].x != AR_NONE_KEY) atomicAdd(&rank_out[r0 + i], cnt_s[i]);
}
