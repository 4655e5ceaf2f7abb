// Ranking: the order of the top-k and the workgroup primitives that every ranking kernel shares -- the key and composite of a
// score, the 12-bit slot hash, the workgroup prefix scan, the radix select and the bitonic sort -- and the dense kernels
// (mask_seen_kernel, topk_seen_kernel).  full_rank.h and sampled_rank.h build on these; all of them run ROW_THREADS threads.
#pragma once
#include "kernels.h"

// Order of the top-k (bsarec_topk_seen, include/bsarec_hip.h): a TOTAL order on (score, column) -- score descending with
// every NaN equal to each other and above +inf, -0 equal to +0; among equal scores the smaller column first.  topk_key maps
// a score to a 32-bit key whose unsigned order is that score order (canonical NaN / +0 first, then the usual sign flip); a
// real score's key is >= topk_key(-inf) = 0x007fffff, so key 0 sorts below every score.
__device__ __forceinline__ unsigned topk_key(float v) {
    unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;          // any NaN -> one quiet NaN (key 0xffc00000 > +inf's)
    if (u == 0x80000000u) u = 0u;                                   // -0 -> +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// The composite of (key, column): its unsigned order is the total order, and composites of different columns are distinct.
__device__ __forceinline__ unsigned long long rank_comp(unsigned key, unsigned col) {
    return ((unsigned long long)key << 32) | (unsigned)~col;
}

// Home slot of an item in an open-addressed LDS table of RANK_SLOTS entries: the top 12 bits of a multiplicative hash.
#define RANK_SLOTS 4096
static_assert(RANK_SLOTS == 1 << 12, "rank_hash: 12 bits");
__device__ __forceinline__ unsigned rank_hash(unsigned x) { return (x * 2654435761u) >> 20; }

// Inclusive prefix of v over the workgroup in thread order (wave scan, then the waves' sums handed over through wscan[]);
// *total, when asked for, is the sum over all threads.  One barrier inside; the caller puts one before wscan is written again.
__device__ __forceinline__ unsigned rank_scan(unsigned* wscan, unsigned v, unsigned* total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v, sum = 0u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned y = __shfl_up(incl, off, 64); if (lane >= off) incl += y; }
    if (lane == 63) wscan[wave] = incl;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < ROW_THREADS / 64; ++w) { const unsigned s = wscan[w]; if (w < wave) incl += s; sum += s; }
    if (total) *total = sum;
    return incl;
}

struct RankRadix { unsigned hist[ROW_THREADS / 64][256]; unsigned wscan[ROW_THREADS / 64]; unsigned sel[3]; };
template <class K> struct RankThreshold { K prefix, mask; int rem; };

// Radix select of the k-th largest of the n keys get(0 .. n), n >= k, K = unsigned (4 digits) or unsigned long long (8):
// 8-bit digits from the most significant one; each pass histograms the digit of the keys that match the prefix chosen so
// far (per-wave LDS histograms; UNROLL: of that loop over the keys), a workgroup scan over the 256 bins (descending digit,
// one thread per bin) picks the bin that holds the k-th key; it stops early once that bin is taken whole.  The result is a
// (prefix, mask) threshold: `rem` keys with key & mask == prefix are still needed, k - rem keys lie above it.  For DISTINCT
// keys, prefix alone is T with #{i : get(i) >= T} == k.  Called by all ROW_THREADS threads; starts and ends with a barrier
// (what the caller wrote to LDS before the call is visible in get and after it), and resets sel every pass.
template <class K, int UNROLL, class N, class F>
__device__ __forceinline__ RankThreshold<K> rank_select(RankRadix& sm, N n, int k, F get) {
    constexpr int NW = ROW_THREADS / 64;
    const int tid = threadIdx.x, wave = tid >> 6;
    RankThreshold<K> t = {0, 0, k};                      // rem: keys still to take among those matching the prefix
    __syncthreads();
    for (int shift = 8 * (int)sizeof(K) - 8; shift >= 0; shift -= 8) {
        for (int i = tid; i < NW * 256; i += ROW_THREADS) (&sm.hist[0][0])[i] = 0u;
        __syncthreads();
        if (tid == 0) { sm.sel[0] = 0u; sm.sel[1] = 0u; sm.sel[2] = 0u; }
#pragma unroll UNROLL
        for (N i = tid; i < n; i += ROW_THREADS) {
            const K v = get(i);
            if ((v & t.mask) == t.prefix) atomicAdd(&sm.hist[wave][(unsigned)(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        const int bin = 255 - tid;                       // thread t owns digit 255 - t: the scan runs from the top digit down
        unsigned cnt = 0u;
#pragma unroll
        for (int w = 0; w < NW; ++w) cnt += sm.hist[w][bin];
        const unsigned incl = rank_scan(sm.wscan, cnt), above = incl - cnt;   // above: matching keys with a larger digit
        if (above < (unsigned)t.rem && incl >= (unsigned)t.rem) { sm.sel[0] = bin; sm.sel[1] = above; sm.sel[2] = cnt; }   // exactly one thread
        __syncthreads();
        t.rem -= (int)sm.sel[1];
        t.prefix |= (K)sm.sel[0] << shift;
        t.mask |= (K)255 << shift;
        if (sm.sel[2] == (unsigned)t.rem) break;         // the bin is taken whole: no finer digit needed
    }
    __syncthreads();
    return t;
}

// Descending bitonic sort of n (a power of two) composites in LDS; VAL: val[] is permuted along with them.  Starts and ends
// with a barrier.
template <bool VAL>
__device__ __forceinline__ void rank_sort(unsigned long long* cand, float* val, int n) {
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (n >> 1); i += ROW_THREADS) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const unsigned long long a = cand[lo], b = cand[hi];
                if (((lo & size) == 0) == (a < b)) {
                    cand[lo] = b; cand[hi] = a;
                    if (VAL) { const float t = val[lo]; val[lo] = val[hi]; val[hi] = t; }
                }
            }
            __syncthreads();
        }
    }
}

// =============================================================================================
// Evaluation: scores of the items a user has already interacted with are set to 0 -- not -inf -- before the top-k
// (src/trainers.py:134: rating_pred[train_matrix[user].toarray() > 0] = 0).  One workgroup per batch row walks the
// user's CSR row on the device.
// =============================================================================================
__global__ void __launch_bounds__(ROW_THREADS)
mask_seen_kernel(float* __restrict__ scores, long ld, const int64_t* __restrict__ users, const int64_t* __restrict__ indptr,
                 const int64_t* __restrict__ indices) {
    const long u = users[blockIdx.x];
    const long j0 = indptr[u], j1 = indptr[u + 1];
    float* row = scores + (long)blockIdx.x * ld;
    for (long j = j0 + threadIdx.x; j < j1; j += ROW_THREADS) row[indices[j]] = 0.f;
}

// Seen-item masking of bsarec_topk_seen: the CSR row of the user is written as zeros into the score row (as the reference does
// -- the caller may still read the masked scores).  Ends with a barrier: the scan that follows reads the zeros.
__device__ __forceinline__ void topk_mask_seen(float* row, int V, const int64_t* users, const int64_t* indptr, const int64_t* indices) {
    if (!indptr) return;
    const long u = users[blockIdx.x];
    const long j0 = indptr[u], j1 = indptr[u + 1];
    for (long j = j0 + threadIdx.x; j < j1; j += ROW_THREADS) { const long it = indices[j]; if (it >= 0 && it < V) row[it] = 0.f; }
    __syncthreads();
}

// Top-k of every score row with the seen items zeroed first, 1 <= k <= TOPK_MAX: the body of the reference's evaluation loop
// for one batch (src/trainers.py:134-149: rating_pred[train_matrix[user] > 0] = 0, np.argpartition(..., -20), argsort of the
// 20) in ONE launch, one workgroup per user.  (1) topk_mask_seen; (2) rank_select of the k-th largest 32-bit key -- keys, not
// composites: at most 4 passes over the V-long row; (3) one ORDERED compaction pass over the row in 256-column chunks: keys
// above the threshold take slots [0, k - rem) through an LDS counter; keys on the threshold are ranked by column (ballot +
// workgroup prefix of the wave counts) and the first rem of them fill slots [k - rem, k) -- exact ties at the k-th place (e.g.
// thousands of seen-item zeros) go to the smaller columns.  (4) rank_sort of the k composites in LDS, padded with 0 (below
// every real key) to a power of two.  Every pass re-reads the row from global memory (L2-resident at these row lengths);
// LDS: 4 KB of histograms + 8 KB of candidates.
#define TOPK_MAX 1024
__global__ void __launch_bounds__(ROW_THREADS)
topk_seen_kernel(float* __restrict__ scores, long ld, int V, const int64_t* __restrict__ users, const int64_t* __restrict__ indptr,
                 const int64_t* __restrict__ indices, int k, int64_t* __restrict__ out_idx, float* __restrict__ out_val) {
    constexpr int NW = ROW_THREADS / 64;
    __shared__ RankRadix sm;
    __shared__ unsigned long long cand[TOPK_MAX];
    __shared__ unsigned wcnt[2][NW], ngt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* row = scores + (long)blockIdx.x * ld;
    topk_mask_seen(row, V, users, indptr, indices);
    if (tid == 0) ngt = 0u;
    for (int i = tid; i < TOPK_MAX; i += ROW_THREADS) cand[i] = 0ull;   // (the sort's padding; the select's barriers order it)
    // ---- (2) radix select
    const RankThreshold<unsigned> th = rank_select<unsigned, 4>(sm, V, k, [&](int c) { return topk_key(row[c]); });
    const unsigned prefix = th.prefix, mask = th.mask;
    const int rem = th.rem;
    // ---- (3) ordered compaction
    const int n_gt = k - rem;
    int taken = 0;                                       // threshold keys ranked so far (the same in every thread)
    for (int c0 = 0, par = 0; c0 < V; c0 += ROW_THREADS, par ^= 1) {
        const int c = c0 + tid;
        const unsigned key = c < V ? topk_key(row[c]) : 0u;
        const unsigned long long comp = rank_comp(key, (unsigned)c);
        if (c < V && (key & mask) > prefix) cand[atomicAdd(&ngt, 1u)] = comp;
        if (taken < rem) {
            const bool eq = c < V && (key & mask) == prefix;
            const unsigned long long bal = __ballot(eq);
            if (lane == 0) wcnt[par][wave] = (unsigned)__popcll(bal);
            __syncthreads();                             // (wcnt is double-buffered: the next chunk writes the other half)
            int before = taken;
#pragma unroll
            for (int w = 0; w < NW; ++w) { const int n = (int)wcnt[par][w]; if (w < wave) before += n; taken += n; }
            if (eq) {
                const int r = before + __popcll(bal & ((1ull << lane) - 1ull));
                if (r < rem) cand[n_gt + r] = comp;
            }
        }
    }
    // ---- (4) bitonic sort of the k survivors, descending
    int n = 1;
    while (n < k) n <<= 1;
    rank_sort<false>(cand, nullptr, n);
    for (int r = tid; r < k; r += ROW_THREADS) {
        const int c = (int)~(unsigned)cand[r];            // (a slot left empty would read -1: never a load out of the row)
        out_idx[(long)blockIdx.x * k + r] = c;
        if (out_val) out_val[(long)blockIdx.x * k + r] = c >= 0 && c < V ? row[c] : __builtin_nanf("");
    }
}
