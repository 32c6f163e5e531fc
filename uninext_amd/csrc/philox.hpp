// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the keep decision of the attention
// dropout inside the bi-directional attention core (include/biattn_hip.h: biattn_hip_train_dropout_f32,
// biattn_hip_backward_dropout_f32, biattn_hip_dropout_keep_u8).  Internal: device code only, not part of the C ABI.
//
// The decision for one entry of an attention matrix is a pure function of (seed, offset, side, b * heads + h, image token i,
// text token j): no tile, range, wave or launch geometry enters, and the forward, both backward passes and the export kernel
// call the SAME function, so the backward reproduces the forward's mask by recomputation and no mask is ever stored.
//
//   key      = (low, high) 32 bits of the seed
//   counter  = (low 32 bits of the offset, high 32 bits of the offset, i, side << 31 | (b * heads + h) << 8 | j / 4)
//              (b * heads + h <= 65535 and j <= 255 by the C ABI's limits, i < 2^30)
//   word t   of the call's four decides entry (i, j = 4 (j / 4) + t);   keep <=> word >= threshold,
//              threshold = (uint32) llrint(p * 2^32), computed once on the host: p = 0 keeps everything
//   side     0: p_v[i, j] (the image side's softmax over the text tokens), 1: p_l[j, i] (the text side's, over the image tokens);
//              it is part of the counter, so the two masks are independent.
//
// GROUPING.  One call decides FOUR CONSECUTIVE TEXT TOKENS of ONE image token, on both sides.  A lane of
// v_mfma_f32_32x32x2_f32 holds four consecutive rows of one column per 8-row group (attn_tile.hpp: register v of lane l is row
// 8 (v / 4) + 4 (l / 32) + v % 4), and the rows are the STREAMED tokens.  The image-owner kernels (image_fwd, bwd_image<*>) stream
// text tokens: registers 4 u .. 4 u + 3 of a lane are one call, four calls a tile and side (keep_bits_image_owner).  The
// text-owner kernels (text_fwd, bwd_text<*>) stream image tokens and hold the tile the other way round: a lane's 16 registers
// are 16 image tokens of ONE text token, so each is a call of its own of which one word is used -- sixteen calls a tile
// (keep_bits_text_owner).  Either grouping serves four of the eight mask uses; this one gives the single calls to the side
// whose kernels carry the two masks at once (bwd_image<false>).
//
// The 16 decisions of a lane's tile are returned as 16 bits, drawn BEFORE the score fragment is live: the kernels around them
// sit at the whole register file, and one register per mask is what stays live across the products.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace philox {

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u;   // the round's two multipliers
constexpr uint32_t kKey0 = 0x9E3779B9u, kKey1 = 0xBB67AE85u;   // the key's two increments (golden ratio, sqrt(3) - 1)

struct Words { uint32_t w[4]; };

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(kMul0, c0), l0 = kMul0 * c0;
    const uint32_t h1 = __umulhi(kMul1, c2), l1 = kMul1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += kKey0;
    k1 += kKey1;
  }
  return {{c0, c1, c2, c3}};
}

// What the kernels take: where the seed and the offset lie on the device, the threshold and the scale of the kept entries.
struct Dropout {
  const unsigned long long* seed;     // [2]: seed, offset
  uint32_t threshold;                 // keep <=> word >= threshold
  float scale;                        // c = 1 / (1 - p), fp32, from the host
};

// the seed and the offset as the four 32-bit words the calls take
struct Stream { uint32_t k0, k1, o0, o1; };

__device__ __forceinline__ Stream stream_of(const Dropout& d) {
  const unsigned long long seed = d.seed[0], offset = d.seed[1];
  return {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
}

constexpr int kSideV = 0, kSideL = 1;

// the four words of entries (i, 4 g .. 4 g + 3) of `side` in (batch, head) bh
__device__ __forceinline__ Words entry_words(const Stream& s, int side, int bh, int i, int g) {
  return philox4x32_10(s.o0, s.o1, (uint32_t)i, (uint32_t)side << 31 | (uint32_t)bh << 8 | (uint32_t)g, s.k0, s.k1);
}

// Image-owner fragment: the lane's image token i, register v = text token j0 + 8 (v / 4) + 4 half + v % 4 (j0 a multiple of 32).
// Bit v of the result: register v is kept.  Four calls.
__device__ __forceinline__ uint32_t keep_bits_image_owner(const Stream& s, uint32_t threshold, int side, int bh, int i, int j0, int half) {
  uint32_t bits = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const Words x = entry_words(s, side, bh, i, (j0 >> 2) + 2 * u + half);
#pragma unroll
    for (int t = 0; t < 4; ++t) bits |= (uint32_t)(x.w[t] >= threshold) << (4 * u + t);
  }
  return bits;
}

// Text-owner fragment: the lane's text token j, register v = image token i0 + 8 (v / 4) + 4 half + v % 4.  Bit v of the result:
// register v is kept.  Sixteen calls, of each the word j % 4.
__device__ __forceinline__ uint32_t keep_bits_text_owner(const Stream& s, uint32_t threshold, int side, int bh, int j, int i0, int half) {
  uint32_t bits = 0;
  const int t = j & 3;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const Words x = entry_words(s, side, bh, i0 + 8 * (v >> 2) + 4 * half + (v & 3), j >> 2);
    const uint32_t w = t == 0 ? x.w[0] : t == 1 ? x.w[1] : t == 2 ? x.w[2] : x.w[3];
    bits |= (uint32_t)(w >= threshold) << v;
  }
  return bits;
}

// Role-neutral names for a self-attention core (bert_attn_common.hpp, bert_attn_bwd.hip: side kSideV, j = key < 512 so that
// j / 4 fits the counter's 8 bits): the matrix's ROW i is the query, its COLUMN j the key.  A kernel that owns rows and streams
// columns draws as the image owner does (four calls a tile), one that owns columns and streams rows as the text owner does
// (sixteen).  The same functions, so the bi-attention core's bits cannot move.
__device__ __forceinline__ uint32_t keep_bits_row_owner(const Stream& s, uint32_t threshold, int bh, int i, int j0, int half) {
  return keep_bits_image_owner(s, threshold, kSideV, bh, i, j0, half);
}
__device__ __forceinline__ uint32_t keep_bits_col_owner(const Stream& s, uint32_t threshold, int bh, int j, int i0, int half) {
  return keep_bits_text_owner(s, threshold, kSideV, bh, j, i0, half);
}

// Row dropout of a [rows, features] activation (include/dynmask_hip.h: dropout_add_layernorm_hip_*, relu_dropout_hip_f32,
// row_dropout_hip_keep_u8): the decision is a pure function of (seed, offset, row, column), no launch geometry enters.
//   key = the seed's two halves, counter = (offset low, offset high, row, column / 4)      (rows < 2^32, features % 4 == 0)
//   word t decides column 4 (column / 4) + t: one call serves the float4 of one lane.  Same threshold rule as above.
__device__ __forceinline__ Words row_words(const Stream& s, uint32_t row, uint32_t col4) {
  return philox4x32_10(s.o0, s.o1, row, col4, s.k0, s.k1);
}

// c where bit v of `bits` is set, else 0: the factor c m of entry v
__device__ __forceinline__ float keep_factor(uint32_t bits, int v, float scale) { return (bits >> v & 1u) ? scale : 0.f; }

}  // namespace philox
