// Full-catalogue top-k without the B x V score matrix (bsarec_topk_full / bsarec_topk_full_range, include/bsarec_hip.h): every
// item is scored on the fly and only the items that can still reach a row's top-k are kept.  The order, the seen-item zeros and
// the result are those of topk_seen_kernel on the materialised matrix.  Launch sequence on one stream (no host synchronisation):
//   (1) full_rank_sample_kernel: score s strided columns per row (seen items as 0), tau_b = a composite no larger than the
//       sample's k-th (key << 32 | ~column) composite -- a lower bound on the row's true k-th composite;
//   (2) full_rank_filter_kernel: (128-row tile x item range) grid, the scores of 128 rows x 32 items per wave by score_tile
//       (score_tile.h); an item survives when its raw composite or its composite as a seen zero is >= tau_b, and is appended
//       (column, raw score) to the row's list with one atomic per half-wave; the count grows past the capacity;
//   (3) FR_ROUNDS x { full_rank_rethreshold_kernel: for an overflowed row, the k-th of min(raw, zero) composites over the
//       first `cap` stored items is a tighter bound; filter again, overflowed rows only (the others keep tau = ~0) };
//   (4) full_rank_select_kernel: rows within capacity: seen candidates set to +0 (LDS hash of the CSR row, 2048 entries per
//       chunk), radix select of the k-th composite, compaction, bitonic sort;
//   (5) full_rank_fallback_kernel: rows still over capacity: exact streaming top-k over 2048-item segments, rescoring the
//       row (seen bits of a segment in LDS), O(k) state.
// Every score is the fmaf chain of fr_dot: acc = 0, then acc = fmaf(h[i], e[i], acc) for i = 0 .. d-1 -- which is what
// score_tile computes bit for bit, so all five kernels see identical scores.
// Column base (bsarec_topk_full_range): E holds rows [base, base + V) of a larger catalogue.  Columns, composites and list
// entries stay LOCAL (0 .. V), so the tie order inside the range is the global one; the base enters where a GLOBAL id crosses
// the interface only: a CSR entry `it` applies iff 0 <= it - base < V, and fr_write adds the base to the ids it stores.
#pragma once
#include "rank.h"
#include "score_tile.h"

#define FR_ROWS 128                        // rows per filter tile: 4 row blocks of the 32 x 32 MFMA
#define FR_ITEMS 128                       // items per filter step: 4 waves x 32
#define FR_ROUNDS 2                        // re-threshold rounds before the fallback
#define FR_HASH RANK_SLOTS                 // select: LDS hash slots (rank_hash) for 2048 seen items per chunk
#define FR_SEG 2048                        // fallback: items per segment
#define FR_KEY0 0x80000000u                // topk_key(+0.0f)

__device__ __forceinline__ unsigned long long fr_entry_comp(unsigned long long e) {   // list entry: score bits << 32 | column
    return rank_comp(topk_key(__uint_as_float((unsigned)(e >> 32))), (unsigned)e);
}
// One score: h row in LDS, item row from global (16-byte aligned, d % 4 == 0).
__device__ __forceinline__ float fr_dot(const float* hs, const float* __restrict__ e, int d) {
    const float4* e4 = reinterpret_cast<const float4*>(e);
    float acc = 0.f;
    for (int q = 0; q < (d >> 2); ++q) {
        const float4 v = e4[q];
        acc = fmaf(hs[4 * q], v.x, acc);
        acc = fmaf(hs[4 * q + 1], v.y, acc);
        acc = fmaf(hs[4 * q + 2], v.z, acc);
        acc = fmaf(hs[4 * q + 3], v.w, acc);
    }
    return acc;
}

// The k-th largest of n DISTINCT composites get(0 .. n), n >= k: T with #{i : get(i) >= T} == k (rank_select; starts and
// ends with a barrier).
template <class N, class F>
__device__ __forceinline__ unsigned long long fr_kth(RankRadix& sm, N n, int k, F get) {
    return rank_select<unsigned long long, 1>(sm, n, k, get).prefix;
}
// A CSR entry g (a GLOBAL id) as a local column of [base, base + V), or -1 when it lies outside.
__device__ __forceinline__ long fr_local(long g, long base, int V) {
    const long it = g >= base ? g - base : -1;
    return it < V ? it : -1;
}
__device__ __forceinline__ void fr_write(const unsigned long long* cand, const float* val, int V, long base, int k,
                                         int64_t* out_idx, float* out_val) {
    for (int r = threadIdx.x; r < k; r += ROW_THREADS) {
        const int c = (int)~(unsigned)cand[r];           // (a slot left empty reads -1)
        out_idx[(long)blockIdx.x * k + r] = c >= 0 ? base + c : c;
        if (out_val) out_val[(long)blockIdx.x * k + r] = c >= 0 && c < V ? val[r] : __builtin_nanf("");
    }
}

// (1) threshold from s columns i * stride, i < s.  skeys: [B][s] keys (the column is implied by the index).
__global__ void __launch_bounds__(ROW_THREADS)
full_rank_sample_kernel(const float* __restrict__ h, long ldh, const float* __restrict__ E, int V, long base, int d,
                        const int64_t* __restrict__ users, const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                        int k, int s, int stride, unsigned* skeys, unsigned long long* tau, unsigned* count) {
    __shared__ float hs[256];
    __shared__ RankRadix sm;
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < d; i += ROW_THREADS) hs[i] = h[(long)b * ldh + i];
    __syncthreads();
    unsigned* keys = skeys + (long)b * s;
    for (int i = tid; i < s; i += ROW_THREADS) keys[i] = topk_key(fr_dot(hs, E + (long)i * stride * d, d));
    __syncthreads();
    if (indptr) {
        const long u = users[b];
        for (long j = indptr[u] + tid; j < indptr[u + 1]; j += ROW_THREADS) {
            const long it = fr_local(indices[j], base, V);
            if (it >= 0 && it % stride == 0 && it / stride < s) keys[it / stride] = FR_KEY0;
        }
    }
    const unsigned long long T = fr_kth(sm, s, k, [&](long i) { return rank_comp(keys[i], (unsigned)(i * stride)); });
    if (tid == 0) { tau[b] = T; count[b] = 0u; }
}

// (2) the filter.  Dynamic LDS: FR_ROWS x (d + 4) floats of h.  list: [B][cap] entries score bits << 32 | column.
__global__ void __launch_bounds__(ROW_THREADS)
full_rank_filter_kernel(const float* __restrict__ h, long ldh, const float* __restrict__ E, int B, int V, int d, int cap,
                        const unsigned long long* __restrict__ tau, unsigned* count, unsigned long long* list) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    __shared__ unsigned long long tau_s[FR_ROWS];
    __shared__ unsigned lo_s[FR_ROWS];
    __shared__ int any;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, half = lane >> 5;
    const int r0 = blockIdx.x * FR_ROWS;
    if (tid == 0) any = 0;
    __syncthreads();
    for (int i = tid; i < FR_ROWS; i += ROW_THREADS) {
        const unsigned long long t = r0 + i < B ? tau[r0 + i] : ~0ull;
        tau_s[i] = t;
        // fast reject below lo: a key under tau's key fails, unless a seen zero at this threshold could pass (lo = 0)
        lo_s[i] = (unsigned)(t >> 32) > FR_KEY0 ? (unsigned)(t >> 32) : 0u;
        if (t != ~0ull) any = 1;
    }
    __syncthreads();
    if (!any) return;                                    // a re-threshold round with no overflowed row in this tile
    score_stage(h, ldh, B, d, r0, FR_ROWS, sh);
    __syncthreads();
    const int nblk = (V + FR_ITEMS - 1) / FR_ITEMS;
    for (int ib = blockIdx.y; ib < nblk; ib += gridDim.y) {
        const unsigned i0 = (unsigned)ib * FR_ITEMS + wave * 32;         // this wave's 32 items
        const int item = (int)i0 + l31;
        const bool iv = item < V;
        unsigned eoff;
        const float* eb = score_items(E, V, d, i0, eoff);
        f32x16 acc[4];
        score_tile<4, false>(sh, eb, eoff, d, acc);
        const unsigned long long zc = rank_comp(FR_KEY0, (unsigned)item);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = rb * 32 + rho(r) + 4 * half;   // row of the tile; column = item
                const float sc = acc[rb][r];
                const unsigned key = topk_key(sc);
                bool pass = false;
                if (iv && key >= lo_s[i]) {
                    const unsigned long long t = tau_s[i];
                    pass = rank_comp(key, (unsigned)item) >= t || zc >= t;
                }
                const unsigned long long bal = __ballot(pass);
                if (bal) {
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const unsigned long long m = bal & (hh ? 0xffffffff00000000ull : 0xffffffffull);
                        if (!m) continue;
                        const int leader = __ffsll((long long)m) - 1;
                        const int row = r0 + rb * 32 + rho(r) + 4 * hh;
                        unsigned base = 0u;
                        if (lane == leader) base = atomicAdd(&count[row], (unsigned)__popcll(m));
                        base = __shfl(base, leader, 64);
                        if (pass && half == hh) {
                            const unsigned slot = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                            if (slot < (unsigned)cap)
                                list[(long)row * cap + slot] = ((unsigned long long)__float_as_uint(sc) << 32) | (unsigned)item;
                        }
                    }
                }
            }
    }
}

// (3) re-threshold: overflowed rows get tau = max(tau, k-th lower bound of the first cap entries) and count 0; the others
// tau = ~0 (the next filter round skips them; their list stays).
__global__ void __launch_bounds__(ROW_THREADS)
full_rank_rethreshold_kernel(int k, int cap, unsigned long long* tau, unsigned* count, const unsigned long long* __restrict__ list) {
    __shared__ RankRadix sm;
    const int b = blockIdx.x;
    const unsigned n = count[b];
    if (n <= (unsigned)cap) { if (threadIdx.x == 0) tau[b] = ~0ull; return; }
    const unsigned long long* L = list + (long)b * cap;
    const unsigned long long T = fr_kth(sm, cap, k, [&](long i) {
        const unsigned long long e = L[i], rc = fr_entry_comp(e), zc = rank_comp(FR_KEY0, (unsigned)e);
        return rc < zc ? rc : zc;
    });
    if (threadIdx.x == 0) { const unsigned long long t = tau[b]; tau[b] = T > t ? T : t; count[b] = 0u; }
}

// (4) rows within capacity.
__global__ void __launch_bounds__(ROW_THREADS)
full_rank_select_kernel(int V, long base, int k, int cap, const int64_t* __restrict__ users, const int64_t* __restrict__ indptr,
                        const int64_t* __restrict__ indices, const unsigned* __restrict__ count, unsigned long long* list,
                        int64_t* __restrict__ out_idx, float* __restrict__ out_val) {
    __shared__ int table[FR_HASH];
    __shared__ unsigned long long cand[TOPK_MAX];
    __shared__ float cval[TOPK_MAX];
    __shared__ unsigned ncand;
    __shared__ RankRadix sm;
    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned n = count[b];
    if (n > (unsigned)cap) return;                      // the fallback's row
    unsigned long long* L = list + (long)b * cap;
    if (indptr) {
        const long u = users[b], j0 = indptr[u], j1 = indptr[u + 1];
        for (long c0 = j0; c0 < j1; c0 += FR_HASH / 2) {
            for (int i = tid; i < FR_HASH; i += ROW_THREADS) table[i] = -1;
            __syncthreads();
            const long c1 = c0 + FR_HASH / 2 < j1 ? c0 + FR_HASH / 2 : j1;
            for (long j = c0 + tid; j < c1; j += ROW_THREADS) {
                const long it = fr_local(indices[j], base, V);
                if (it < 0) continue;
                for (unsigned p = rank_hash((unsigned)it);; p = (p + 1) & (FR_HASH - 1)) {
                    const int old = atomicCAS(&table[p], -1, (int)it);
                    if (old == -1 || old == (int)it) break;
                }
            }
            __syncthreads();
            for (unsigned i = tid; i < n; i += ROW_THREADS) {
                const int col = (int)(unsigned)L[i];
                for (unsigned p = rank_hash((unsigned)col);; p = (p + 1) & (FR_HASH - 1)) {
                    const int t = table[p];
                    if (t == col) { L[i] = (unsigned)col; break; }   // seen: score +0.0
                    if (t == -1) break;
                }
            }
            __syncthreads();
        }
    }
    const unsigned long long T = fr_kth(sm, n, k, [&](long i) { return fr_entry_comp(L[i]); });
    for (int i = tid; i < TOPK_MAX; i += ROW_THREADS) cand[i] = 0ull;
    if (tid == 0) ncand = 0u;
    __syncthreads();
    for (unsigned i = tid; i < n; i += ROW_THREADS) {
        const unsigned long long e = L[i], c = fr_entry_comp(e);
        if (c >= T) {
            const unsigned slot = atomicAdd(&ncand, 1u);
            if (slot < (unsigned)k) { cand[slot] = c; cval[slot] = __uint_as_float((unsigned)(e >> 32)); }
        }
    }
    int np = 1;
    while (np < k) np <<= 1;
    rank_sort<true>(cand, cval, np);
    fr_write(cand, cval, V, base, k, out_idx, out_val);
}

// (5) rows over capacity after the last round: exact streaming top-k, segment by segment.
__global__ void __launch_bounds__(ROW_THREADS)
full_rank_fallback_kernel(const float* __restrict__ h, long ldh, const float* __restrict__ E, int V, long base, int d, int k,
                          int cap, const int64_t* __restrict__ users, const int64_t* __restrict__ indptr,
                          const int64_t* __restrict__ indices, const unsigned* __restrict__ count,
                          int64_t* __restrict__ out_idx, float* __restrict__ out_val) {
    __shared__ float hs[256];
    __shared__ unsigned long long cur[TOPK_MAX], seg[FR_SEG];
    __shared__ float curv[TOPK_MAX], segv[FR_SEG];
    __shared__ unsigned bits[FR_SEG / 32];
    __shared__ unsigned nsel;
    __shared__ RankRadix sm;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (count[b] <= (unsigned)cap) return;
    for (int i = tid; i < d; i += ROW_THREADS) hs[i] = h[(long)b * ldh + i];
    long j0 = 0, j1 = 0;
    if (indptr) { const long u = users[b]; j0 = indptr[u]; j1 = indptr[u + 1]; }
    int ncur = 0;
    for (int c0 = 0; c0 < V; c0 += FR_SEG) {
        const int m = V - c0 < FR_SEG ? V - c0 : FR_SEG;
        for (int i = tid; i < FR_SEG / 32; i += ROW_THREADS) bits[i] = 0u;
        __syncthreads();
        for (long j = j0 + tid; j < j1; j += ROW_THREADS) {
            const long it = fr_local(indices[j], base, V);
            if (it >= c0 && it < c0 + m) atomicOr(&bits[(it - c0) >> 5], 1u << ((it - c0) & 31));
        }
        __syncthreads();
        for (int t = tid; t < m; t += ROW_THREADS) {
            const float sc = (bits[t >> 5] >> (t & 31)) & 1u ? 0.f : fr_dot(hs, E + (long)(c0 + t) * d, d);
            seg[t] = rank_comp(topk_key(sc), (unsigned)(c0 + t));
            segv[t] = sc;
        }
        __syncthreads();
        if (ncur + m <= k) {                            // fewer than k items so far: keep them all
            for (int t = tid; t < m; t += ROW_THREADS) { cur[ncur + t] = seg[t]; curv[ncur + t] = segv[t]; }
            ncur += m;
            __syncthreads();
            continue;
        }
        const unsigned long long T = fr_kth(sm, ncur + m, k, [&](long i) { return i < ncur ? cur[i] : seg[i - ncur]; });
        // survivors: first those of cur (compacted in place, to the front), then those of seg
        if (tid == 0) nsel = 0u;
        __syncthreads();
        constexpr int KP = TOPK_MAX / ROW_THREADS;       // cur entries per thread (ncur <= k <= TOPK_MAX)
        unsigned long long keep_c[KP];
        float keep_v[KP];
#pragma unroll
        for (int q = 0; q < KP; ++q) {
            const int i = tid + q * ROW_THREADS;
            keep_c[q] = i < ncur ? cur[i] : 0ull;
            keep_v[q] = i < ncur ? curv[i] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < KP; ++q)
            if (keep_c[q] >= T && keep_c[q] != 0ull) {
                const unsigned slot = atomicAdd(&nsel, 1u);
                if (slot < (unsigned)k) { cur[slot] = keep_c[q]; curv[slot] = keep_v[q]; }
            }
        for (int t = tid; t < m; t += ROW_THREADS)
            if (seg[t] >= T) { const unsigned slot = atomicAdd(&nsel, 1u); if (slot < (unsigned)k) { cur[slot] = seg[t]; curv[slot] = segv[t]; } }
        ncur = k;
        __syncthreads();
    }
    int np = 1;
    while (np < k) np <<= 1;
    for (int i = ncur + tid; i < np; i += ROW_THREADS) cur[i] = 0ull;
    rank_sort<true>(cur, curv, np);
    fr_write(cur, curv, V, base, k, out_idx, out_val);
}
