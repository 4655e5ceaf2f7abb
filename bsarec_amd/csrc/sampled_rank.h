// Sampled-candidate evaluation (bsarec_sampled_rank, include/bsarec_hip.h): per evaluation row, draw N negatives the user
// has not seen from a Philox stream, score the answer and the N negatives against the last-position hidden state, and rank
// the answer among them.  One 256-thread workgroup per row; the protocol (draw stream, acceptance, tie rule) is the
// header's, restated in numpy by tests/sampled_eval_ref.py.
#pragma once
#include "rank.h"

#define NEG_MAX 1024                      // BSAREC_NEG_MAX: the largest N
#define NEG_MAX_DRAWS (1 << 20)           // BSAREC_NEG_MAX_DRAWS: draws examined before a row fails
#define NEG_SLOTS RANK_SLOTS              // dedup table (rank_hash): <= N accepted + <= 1024 draws of one round, load <= 1/2
#define NEG_SEEN_LDS 2048                 // seen rows up to this length are staged in LDS (longer: searched in global memory)

static_assert(NEG_SLOTS >= 4 * NEG_MAX, "sampled_rank: the dedup table's load");
static_assert(NEG_MAX_DRAWS % (ROW_THREADS * 4) == 0 && NEG_MAX_DRAWS % (ROW_THREADS * 2) == 0, "sampled_rank: whole rounds");

// smallest i in [0, V) with cum[i] > r, or V if there is none
__device__ __forceinline__ int neg_upper_bound(const int64_t* __restrict__ cum, int V, int64_t r) {
    int lo = 0, hi = V;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <typename T>
__device__ __forceinline__ bool neg_in_sorted(const T* s, long n, long x) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if ((long)s[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && (long)s[lo] == x;
}

// Sampling runs in rounds of ROW_THREADS Philox calls, thread t making call j = round * ROW_THREADS + t (uniform: 4 draws per
// call, popularity: 2), so a thread's draws are consecutive in the stream and thread order is stream order.  A draw is
// ELIGIBLE when its item is neither the answer nor in the user's (sorted) seen row.  Eligible draws claim their item's slot of
// an open-addressed LDS table (linear probing, CAS on the key) and atomicMin (stream index + 1) into it; after a barrier a
// draw is accepted iff it holds its slot's minimum -- the first draw of an item in stream order.  A slot filled in an
// earlier round keeps that round's (smaller) index, so items accepted before are never accepted again, and every item of a
// non-final round that wins is accepted (truncation at N only happens in the round that ends the sampling): the table holds
// the accepted items plus one round's draws and is never cleared.  The accepted draws of a round are placed in stream order by
// a workgroup prefix scan of the per-thread counts, truncated at N.  Scoring: LPR = the power of two >= d / 4 lanes per
// candidate, one float4 of h (in LDS) and of the item row per lane, a butterfly sum -- the same code for the answer and the
// negatives.  Rank: a workgroup count against the answer's score.
__global__ void __launch_bounds__(ROW_THREADS)
sampled_rank_kernel(const float* __restrict__ h, long ldh, const float* __restrict__ E, int V, int d,
                    const int64_t* __restrict__ users, const int64_t* __restrict__ answers, const int64_t* __restrict__ indptr,
                    const int64_t* __restrict__ indices, const int64_t* __restrict__ pop_cum, int n_neg, uint32_t k0, uint32_t k1,
                    uint32_t tag, int32_t* __restrict__ rank_out, int64_t* __restrict__ cand_out, float* __restrict__ score_out) {
    constexpr int NW = ROW_THREADS / 64;
    __shared__ __attribute__((aligned(16))) float hs[256];
    __shared__ unsigned key[NEG_SLOTS], val[NEG_SLOTS];
    __shared__ int seen_s[NEG_SEEN_LDS];
    __shared__ int cand[NEG_MAX + 1];
    __shared__ float sc[NEG_MAX + 1];
    __shared__ unsigned wsum[NW];
    __shared__ int nrank;
    const int tid = threadIdx.x, lane = tid & 63;
    const long b = blockIdx.x;
    const int64_t u = users[b], a64 = answers[b];
    const bool ans_ok = a64 >= 1 && a64 < V;
    const int a = ans_ok ? (int)a64 : 0;
    long j0 = 0, ns = 0;
    if (indptr) { j0 = indptr[u]; ns = indptr[u + 1] - j0; if (ns < 0) ns = 0; }
    const bool seen_lds = ns <= NEG_SEEN_LDS;
    if (seen_lds)                                        // (a monotone clamp to int keeps the staged row sorted)
        for (int i = tid; i < ns; i += ROW_THREADS) { const int64_t x = indices[j0 + i]; seen_s[i] = x < 0 ? -1 : (x > 0x7fffffff ? 0x7fffffff : (int)x); }
    for (int i = tid; i < NEG_SLOTS; i += ROW_THREADS) { key[i] = 0u; val[i] = 0xffffffffu; }     // key 0: empty (item 0 is never drawn)
    for (int i = tid; i < d; i += ROW_THREADS) hs[i] = h[b * ldh + i];
    if (tid == 0) { cand[0] = a; nrank = 0; }
    const bool pop = pop_cum != nullptr;
    const int64_t T = pop ? pop_cum[V - 1] : 0;
    const int per = pop ? 2 : 4;                         // draws per Philox call
    const int rounds = (ans_ok && (!pop || T >= 1)) ? NEG_MAX_DRAWS / (ROW_THREADS * per) : 0;
    __syncthreads();
    int acc = 0;                                         // negatives accepted so far (the same in every thread)
    for (int r = 0; r < rounds && acc < n_neg; ++r) {
        const uint32_t j = (uint32_t)(r * ROW_THREADS + tid);
        const uint4 w = philox4x32_10(j, (uint32_t)u, (uint32_t)((uint64_t)u >> 32), tag, k0, k1);
        int item[4];
        if (!pop) {
            const uint64_t vm1 = (uint64_t)(V - 1);
            item[0] = 1 + (int)(((uint64_t)w.x * vm1) >> 32); item[1] = 1 + (int)(((uint64_t)w.y * vm1) >> 32);
            item[2] = 1 + (int)(((uint64_t)w.z * vm1) >> 32); item[3] = 1 + (int)(((uint64_t)w.w * vm1) >> 32);
        } else {
            const uint64_t x0 = (uint64_t)w.x | ((uint64_t)w.y << 32), x1 = (uint64_t)w.z | ((uint64_t)w.w << 32);
            item[0] = neg_upper_bound(pop_cum, V, (int64_t)__umul64hi(x0, (uint64_t)T));
            item[1] = neg_upper_bound(pop_cum, V, (int64_t)__umul64hi(x1, (uint64_t)T));
            item[2] = item[3] = 0;
        }
        unsigned slot[4];
        bool elig[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int it = item[m];
            bool e = m < per && it >= 1 && it < V && it != a;
            if (e && ns > 0) e = seen_lds ? !neg_in_sorted(seen_s, ns, it) : !neg_in_sorted(indices + j0, ns, it);
            elig[m] = e;
            slot[m] = rank_hash((unsigned)it);
            if (e) {
                for (;;) {                               // at most 2 * NEG_MAX keys in NEG_SLOTS slots: an empty slot exists
                    const unsigned prev = atomicCAS(&key[slot[m]], 0u, (unsigned)it);
                    if (prev == 0u || prev == (unsigned)it) break;
                    slot[m] = (slot[m] + 1u) & (NEG_SLOTS - 1);
                }
                atomicMin(&val[slot[m]], j * per + m + 1u);
            }
        }
        __syncthreads();
        bool win[4];
        unsigned nwin = 0u;
#pragma unroll
        for (int m = 0; m < 4; ++m) { win[m] = elig[m] && val[slot[m]] == j * per + m + 1u; nwin += win[m] ? 1u : 0u; }
        unsigned total;
        const unsigned before = rank_scan(wsum, nwin, &total) - nwin;
        int pos = acc + (int)before;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (win[m]) { if (pos < n_neg) cand[1 + pos] = item[m]; ++pos; }
        acc = min(n_neg, acc + (int)total);
        __syncthreads();                                 // (wsum and the table's minima are rewritten by the next round)
    }
    // ---- scores of the n_neg + 1 candidates
    const bool ok = acc == n_neg;                        // (false for an answer outside [1, V) too: no round ran)
    const int nc = n_neg + 1, nf4 = d >> 2;
    int lpr = 1;
    while (lpr < nf4) lpr <<= 1;                         // <= 64: d <= 256
    const int grp = tid / lpr, l = tid & (lpr - 1), ngrp = ROW_THREADS / lpr;
    if (ok) {
        for (int c0 = 0; c0 < nc; c0 += ngrp) {          // (a trip count the same in every lane: the butterfly below)
            const int c = c0 + grp;
            float p = 0.f;
            if (c < nc && l < nf4) {
                const f32x4 e = ld4(E + (long)cand[c] * d + 4 * l), hv = ld4(hs + 4 * l);
                p = hv.x * e.x + hv.y * e.y + hv.z * e.z + hv.w * e.w;
            }
            for (int off = lpr >> 1; off > 0; off >>= 1) p += __shfl_xor(p, off, 64);
            if (c < nc && l == 0) sc[c] = p;
        }
        __syncthreads();
        // ---- rank: negatives that score above the answer, equal to it, or NaN
        const float sa = sc[0];
        int cnt = 0;
        for (int i = 1 + tid; i <= n_neg; i += ROW_THREADS) { const float s = sc[i]; cnt += (s > sa || s == sa || s != s) ? 1 : 0; }
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if (lane == 0 && cnt) atomicAdd(&nrank, cnt);
        __syncthreads();
        if (tid == 0) rank_out[b] = sa != sa ? n_neg : nrank;
    } else if (tid == 0) {
        rank_out[b] = -1;
    }
    const long o = b * nc;
    if (cand_out)
        for (int i = tid; i < nc; i += ROW_THREADS) cand_out[o + i] = i == 0 ? a64 : (i <= acc ? (int64_t)cand[i] : 0);
    if (score_out)
        for (int i = tid; i < nc; i += ROW_THREADS) score_out[o + i] = ok ? sc[i] : __builtin_nanf("");
}
