// Keep-bits of a training step's dropout masks (plan option drop_bits).  The forward block kernels evaluate
// every mask once (Philox, common.h) and leave one bit per element here; the matching backward reads the bits instead of
// evaluating Philox a second time.  A bit says "kept": the multiplier is `scale` where it is set and 0 where it is not --
// the two values drop_mult4 / drop_mult1 return, so every result is the same bit for bit.
//
// One buffer per layer, T = B L tokens, everything addressed as a BIT index into it (bit i = bit i & 7 of byte i >> 3):
//   hidden-size sites, slot s (DB_EMBED: the embedding front-end, bottom block only; DB_F, DB_O, DB_FF: the block's
//   drop_f, drop_o, drop_ff), element (token, column c):
//       one byte per group of 4 columns at byte (s T + token) 16 + c / 4, bit c & 3            (16 B per token row and slot)
//     -- the byte is the lane's: the row passes of both kernels hold columns c4 .. c4 + 3, c4 = (tid & 15) << 2, of a row.
//   attention site, element (b, head, query, key):
//       one 16-bit word per (key tile kt = key / 32, half = (key / 4) & 1, query) at word
//       (((b heads + head) 2 + kt) 2 + half) 64 + query behind the hidden slots, bit 4 ((key / 8) & 3) + (key & 3)
//     -- the word is the lane's: forward phase 3 and backward stage C1 hold tile (head, query tile, kt) as lane = query
//        with 16 registers at keys 32 kt + 8 g + 4 half + j (bit 4 g + j).
// The one-row top block writes and reads row L - 1 / query L - 1 of the same layout.
// Host and device share this file (as wimage.h): the kernels, the C ABI's index functions and the tests go through it.
#pragma once
#include "common.h"

enum { DB_EMBED = 0, DB_F = 1, DB_O = 2, DB_FF = 3, DB_SLOTS = 4 };

// byte of (slot, token, columns c4 .. c4 + 3)
__host__ __device__ inline long drop_bits_hidden_byte(int slot, long T, long token, int c4) {
    return ((long)slot * T + token) * 16 + (c4 >> 2);
}
// first byte of the attention words
__host__ __device__ inline long drop_bits_attn_base(long T) { return (long)DB_SLOTS * T * 16; }
// 16-bit word (index, not byte) of (b, head, key tile, half, query) behind drop_bits_attn_base
__host__ __device__ inline long drop_bits_attn_word(int heads, long b, int head, int kt, int half, int query) {
    return (((b * heads + head) * 2 + kt) * 2 + half) * 64 + query;
}
// bytes of one layer's buffer
__host__ __device__ inline long drop_bits_layer_bytes(long B, long L, int heads) {
    return drop_bits_attn_base(B * L) + B * heads * 256 * 2;
}
// the same map element by element, as bit indices (host arithmetic: the C ABI's bsarec_drop_bits_*_bit, the tests)
__host__ __device__ inline long drop_bits_hidden_bit(int slot, long T, long token, int c) {
    return drop_bits_hidden_byte(slot, T, token, c & ~3) * 8 + (c & 3);
}
__host__ __device__ inline long drop_bits_attn_bit(long T, int heads, long b, int head, int query, int key) {
    return (drop_bits_attn_base(T) + 2 * drop_bits_attn_word(heads, b, head, key >> 5, (key >> 2) & 1, query)) * 8 +
           4 * ((key >> 3) & 3) + (key & 3);
}

// ---- device side -----------------------------------------------------------------------------
#define DB_GLOBAL __attribute__((address_space(1)))
// keep bits of a multiplier quad.  A multiplier is `scale` (= 1 / (1 - p) >= 1) or +0.f, so clamping it to [0, 1] (one v_med3_f32) gives the keep bit as a float
// and the four are packed by three exact FMAs and one conversion: eight vector instructions, no comparison (each of which would
// hold a pair of scalar registers, and the forward kernel has none to spare)
__device__ __forceinline__ unsigned drop_keep4(const f32x4& m) {
    float t = __builtin_amdgcn_fmed3f(m.w, 0.0f, 1.0f);
    t = fmaf(t, 2.0f, __builtin_amdgcn_fmed3f(m.z, 0.0f, 1.0f));
    t = fmaf(t, 2.0f, __builtin_amdgcn_fmed3f(m.y, 0.0f, 1.0f));
    t = fmaf(t, 2.0f, __builtin_amdgcn_fmed3f(m.x, 0.0f, 1.0f));
    return (unsigned)t;
}
// ... and back: the multipliers drop_mult4 returned for them
__device__ __forceinline__ f32x4 drop_expand4(unsigned keep, float scale) {
    return f32x4{(keep & 1u) ? scale : 0.f, (keep & 2u) ? scale : 0.f, (keep & 4u) ? scale : 0.f, (keep & 8u) ? scale : 0.f};
}
// Accesses: a wave-uniform base (the block's first row of a slot, a head's first word: scalar registers) plus a small
// per-lane byte offset -- one vector register of address, not a 64-bit pair per request.
__device__ __forceinline__ unsigned drop_bits_ld8(const unsigned char* base, unsigned off) { return *((const DB_GLOBAL unsigned char*)base + off); }
__device__ __forceinline__ unsigned drop_bits_ld16(const unsigned char* base, unsigned off) { return *(const DB_GLOBAL unsigned short*)((const DB_GLOBAL unsigned char*)base + off); }
__device__ __forceinline__ void drop_bits_st8(unsigned char* base, unsigned off, unsigned v) { *((DB_GLOBAL unsigned char*)base + off) = (unsigned char)v; }
__device__ __forceinline__ void drop_bits_st16(unsigned char* base, unsigned off, unsigned v) { *(DB_GLOBAL unsigned short*)((DB_GLOBAL unsigned char*)base + off) = (unsigned short)v; }
// per-lane offsets behind the bases  bits + drop_bits_hidden_byte(slot, T, tok0, 0)  and
// bits + drop_bits_attn_base(T) + 2 drop_bits_attn_word(heads, b, head, 0, 0, 0)
__device__ __forceinline__ unsigned drop_bits_row_off(int row, int c4) { return (unsigned)(row * 16 + (c4 >> 2)); }
__device__ __forceinline__ unsigned drop_bits_word_off(int kt, int half, int query) { return (unsigned)(2 * ((kt * 2 + half) * 64 + query)); }
// A plan keeps bits where it hands the kernels a buffer; with dropout off (eval, p = 0) nothing is evaluated, stored or read.
__device__ __forceinline__ bool drop_bits_live(const DropP& d, const unsigned char* bits) { return bits != nullptr && d.thresh != 0; }

// backward, hidden-size site, in two pieces: the request (placed with the stage's other operands) and the multipliers.
// DB is a compile-time property of the backward kernel: with both the bits and Philox in one body the register allocator has to
// provide for Philox, and the backward has no registers to spare.
template <bool DB>
__device__ __forceinline__ unsigned drop_bits_request(const DropP& d, const unsigned char* base, unsigned off) {
    if constexpr (DB) return d.thresh != 0 ? drop_bits_ld8(base, off) : 0u;
    else return 0u;
}
template <bool DB>
__device__ __forceinline__ f32x4 drop_mult4_saved(const DropP& d, const DropSeed& sd, uint64_t grp, unsigned keep) {
    if constexpr (!DB) return drop_mult4(d, sd, grp);
    else return d.thresh == 0 ? f32x4{d.scale, d.scale, d.scale, d.scale} : drop_expand4(keep, d.scale);
}
