// BERT4Rec's masking step on the device (bsarec_cloze_mask, include/bsarec_hip.h): a Philox draw per token, the masked ids,
// and the compacted list of loss positions that the cloze head (ce_head.h with a row list) reads.
//
// Draw.  Token e = b L + t takes word e & 3 of Philox call (lo32(e >> 2), hi32(e >> 2), BSAREC_CLOZE_SITE, lo32(state[1]))
// keyed by state[0]: the stream of oracle.dropout_keep(B L, ratio, seed, step, BSAREC_CLOZE_SITE), at a site no dropout mask
// uses.  drawn = ids > 0 && word < thresh (thresh = floor(ratio 2^32), at most 2^32 - 1).  A sequence that draws nothing
// and ends in a real item draws its last position.  The loss positions of a sequence are its last min(drawn, slots) drawn ones.
//
// Two launches, no atomics, no scratch beside the outputs themselves:
//   cloze_draw_kernel     a wave per sequence, 64 positions per pass: ballot -> the drawn positions as bit masks, popcounts
//                         for a position's rank among them; masked_ids; the sequence's loss positions, ascending, staged in
//                         rows[b slots ..], -1 behind them
//   cloze_compact_kernel  one workgroup of 1024 lanes walks the staged list 1024 entries at a time in index order: the live
//                         entries move to the front IN PLACE (an entry's target index is never behind its own, and a pass
//                         reads its entries before a barrier and writes after it, so nothing is overwritten before it is
//                         read); targets = ids at the token; then -1 / 0 behind the n live rows, and count[0] = n
// The staged order is (sequence, position) ascending, i.e. token index ascending: the compaction keeps it.
#pragma once
#include "common.h"

#define CLOZE_THREADS 256                   // draw kernel: four sequences per workgroup

struct ClozeP {
    const int64_t* ids; int B, L, slots; uint32_t thresh; int64_t mask_token; const uint64_t* state;
    int64_t* masked_ids; int32_t* rows; int64_t* targets; int32_t* count;
};

__device__ __forceinline__ int cloze_popc(uint64_t m) { return __popcll((unsigned long long)m); }

__global__ void __launch_bounds__(CLOZE_THREADS) cloze_draw_kernel(const ClozeP P) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (CLOZE_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= P.B) return;                                        // (whole waves: no barrier in this kernel)
    const uint64_t seed = P.state[0];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), step = (uint32_t)P.state[1];
    const int npass = (P.L + 63) >> 6;                           // <= 4
    uint64_t drawn[4] = {0, 0, 0, 0};
    int64_t id[4] = {0, 0, 0, 0};
    int total = 0;
    bool last_real = false;                                      // this lane holds position L - 1, a real item
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c >= npass) break;
        const int t = 64 * c + lane;
        bool d = false;
        if (t < P.L) {
            const uint64_t e = (uint64_t)b * P.L + t;
            id[c] = P.ids[e];
            const uint4 w = philox4x32_10((uint32_t)(e >> 2), (uint32_t)(e >> 34), BSAREC_CLOZE_SITE, step, k0, k1);
            const uint32_t word = (e & 3) == 0 ? w.x : (e & 3) == 1 ? w.y : (e & 3) == 2 ? w.z : w.w;
            d = id[c] > 0 && word < P.thresh;
            last_real |= t == P.L - 1 && id[c] > 0;
        }
        drawn[c] = __ballot(d);
        total += cloze_popc(drawn[c]);
    }
    if (total == 0) {                                            // nothing drawn: the last position, if it is a real item
        const uint64_t last = __ballot(last_real);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c == npass - 1) drawn[c] = last;
        total = cloze_popc(last);
    }
    const int keep = total < P.slots ? total : P.slots, skip = total - keep;       // the last `keep` drawn positions carry a loss
    int before = 0;                                              // drawn positions in the passes in front of this one
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c >= npass) break;
        const int t = 64 * c + lane;
        if (t < P.L) {
            const bool d = (drawn[c] >> lane) & 1;
            const long e = (long)b * P.L + t;
            P.masked_ids[e] = d ? P.mask_token : id[c];
            const int rank = before + cloze_popc(drawn[c] & (((uint64_t)1 << lane) - 1));
            if (d && rank >= skip) P.rows[(long)b * P.slots + (rank - skip)] = (int32_t)e;
        }
        before += cloze_popc(drawn[c]);
    }
    for (int i = keep + lane; i < P.slots; i += 64) P.rows[(long)b * P.slots + i] = -1;
}

__global__ void __launch_bounds__(1024) cloze_compact_kernel(const ClozeP P) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = P.B * P.slots;
    int n = 0;                                                   // live rows in front of this pass (the same in every lane)
    for (int s0 = 0; s0 < R; s0 += 1024) {
        const int s = s0 + tid;
        const int v = s < R ? P.rows[s] : -1;
        const bool live = v >= 0;
        const uint64_t bal = __ballot(live);
        if (lane == 0) wsum[wave] = cloze_popc(bal);
        __syncthreads();                                         // every entry of the pass is read; the waves' counts are there
        int base = n, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int c = wsum[w]; if (w < wave) base += c; all += c; }
        if (live) {
            const int r = base + cloze_popc(bal & (((uint64_t)1 << lane) - 1));        // r <= s
            P.rows[r] = v;
            P.targets[r] = P.ids[v];
        }
        n += all;
        __syncthreads();                                         // wsum is free again
    }
    for (int r = n + tid; r < R; r += 1024) { P.rows[r] = -1; P.targets[r] = 0; }
    if (tid == 0) P.count[0] = n;
}
