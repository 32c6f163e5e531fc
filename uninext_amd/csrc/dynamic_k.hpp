// The dynamic-k (simOTA) assignment of one image by one workgroup, shared by ota.hip (matcher.py:387-435) and reid.hip
// (pos_neg_select.py:187-218), and the per-image offsets both files' launchers take.  Internal, not part of the C ABI.
//
// Every float comparison in here decides an integer output, so the INCLUDING FILE MUST HAVE CONTRACTION OFF
// (`#pragma clang fp contract(off)` above the include): an FMA rounds once where the reference's two kernels round twice.  The
// in-place penalties are float32 adds on the stored matrix in the reference's sequence (adding 100000 to a row can MERGE two
// nearby costs into a tie, which the lowest-index rule then decides -- so the adds cannot be folded away).  Selections (top-k,
// argmin, argmax) break ties towards the lowest index, PyTorch's documented rule for min / max with indices and what its
// sort-based top-k does for equal keys.
//
// NaN costs (0 / 0 IoU of two zero-area boxes).  PyTorch's top-k sorts NaN behind everything (nan_to_inf); its min / argmin
// PROPAGATE NaN -- the first NaN of a row or column is "the minimum" (nan_first; a real -inf beside a NaN ties with it here and
// the lower index wins: the one place this code does not follow PyTorch, on inputs no detector produces).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ota_hip.h"
#include "launch_glue.hpp"
#include "wave_ops.hpp"

namespace msda {

__device__ __forceinline__ float nan_to_inf(float v) { return v != v ? INFINITY : v; }
__device__ __forceinline__ float nan_first(float v) { return v != v ? -INFINITY : v; }

constexpr float kTakenPenalty = 100000.0f;      // matcher.py:415, pos_neg_select.py:210
constexpr int kMaxGt = 4096;                    // targets of one image (unmatched flags live in LDS)
constexpr uint8_t kMatch = 1, kStale = 2;       // bit 0 of M[q, g]; bit 1 of M[q, 0]: the row was multiply claimed before the repair loop

// dynamic_k_matching(cost, iou, ncand) of one image by its whole workgroup of kThreads: M [Q, G] is zeroed and filled with the
// final 0 / 1 matrix; C is modified in place as the reference modifies it.  kHasValid: V[g] == 0 means column g does not exist
// (at least one column does); without it V is not read and all G > 0 columns exist.  s_unmatched [kMaxGt] and s_count [2] are
// LDS.  Returns status bit 1 (2) when the repair loop was cut off.  Every thread of the workgroup calls it; it ends behind a
// barrier.
template <bool kHasValid, int kThreads>
__device__ int dynamic_k(float* __restrict__ C, const float* __restrict__ I, uint8_t* __restrict__ M, const uint8_t* __restrict__ V,
                         int Q, int G, int ncand, int max_rounds, uint8_t* s_unmatched, int* s_count) {
  constexpr int kWaves = kThreads / 64;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto exists = [&](int g) { return !kHasValid || V[g] != 0; };
  // a row's cheapest target (torch.min(cost[rows], dim=1): the first minimum of the existing columns) replaces everything the row holds
  auto keep_cheapest = [&](int q) {
    float best = 0.0f;
    int arg = -1;
    for (int g = 0; g < G; ++g) {
      if (!exists(g)) continue;
      const float v = nan_first(C[(int64_t)q * G + g]);
      if (arg < 0 || v < best) { best = v; arg = g; }
    }
    const uint8_t stale = M[(int64_t)q * G] & kStale;
    for (int g = 0; g < G; ++g) M[(int64_t)q * G + g] = 0;
    if (arg >= 0) M[(int64_t)q * G + arg] = kMatch;
    M[(int64_t)q * G] |= stale;
  };
  auto row_sum = [&](int q) {                     // (an absent column never holds a match)
    int n = 0;
    for (int g = 0; g < G; ++g) n += M[(int64_t)q * G + g] & kMatch;
    return n;
  };

  for (int q = tid; q < Q; q += kThreads)
    for (int g = 0; g < G; ++g) M[(int64_t)q * G + g] = 0;
  __syncthreads();

  // ---- dynamic k per target and its k cheapest queries (matcher.py:390-402) -------------------------------------------------
  for (int g = wv; g < G; g += kWaves) {
    if (!exists(g)) continue;
    // the ncand largest IoUs of the column, in descending order; their sum in that order
    float prev_v = INFINITY, sum = 0.0f;
    int prev_i = -1;
    bool has_nan = false;
    for (int r = 0; r < ncand; ++r) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int q = lane; q < Q; q += 64) {
        const float v = I[(int64_t)q * G + g];
        if (!(v == v)) { has_nan = true; continue; }           // (0 / 0 of two zero-area boxes; see k below)
        const bool after = v < prev_v || (v == prev_v && q > prev_i);
        if (after && (v > bv || (v == bv && q < bi))) { bv = v; bi = q; }
      }
      wave_ops::wave_argmax(bv, bi);
      if (bi == 0x7fffffff) break;
      sum = sum + bv;
      prev_v = bv; prev_i = bi;
    }
    // torch.clamp(topk_ious.sum(0).int(), min=1).  torch.topk ranks NaN LARGEST: a column with a NaN IoU has it among its
    // candidates, the sum is NaN, .int() of NaN is 0 (GPU) or INT_MIN (CPU), the clamp makes it 1
    const int k = __any(has_nan) ? 1 : max((int)sum, 1);
    // the k cheapest queries of the column claim the target (torch.topk(cost[:, g], k, largest=False))
    float pv = -INFINITY;
    int pi = -1;
    for (int r = 0; r < k; ++r) {
      float bv = INFINITY;
      int bi = 0x7fffffff;
      for (int q = lane; q < Q; q += 64) {
        const float v = nan_to_inf(C[(int64_t)q * G + g]);
        const bool after = v > pv || (v == pv && q > pi);
        if (after && (v < bv || (v == bv && q < bi))) { bv = v; bi = q; }
      }
      wave_ops::wave_argmin(bv, bi);
      if (bi == 0x7fffffff) break;                              // k > Q cannot happen (k <= ncand terms <= 1 each, ncand <= Q), kept for safety
      if (lane == 0) M[(int64_t)bi * G + g] = kMatch;
      pv = bv; pi = bi;
    }
  }
  __syncthreads();

  // ---- a query claimed by several targets keeps its cheapest one; the set of such rows is remembered (matcher.py:406-411) ---
  for (int q = tid; q < Q; q += kThreads) {
    if (row_sum(q) > 1) {
      keep_cheapest(q);
      M[(int64_t)q * G] |= kStale;
    }
  }
  __syncthreads();

  // ---- repair loop (matcher.py:417-435) ---------------------------------------------------------------------------------------
  int st = 0;
  for (int round = 0;; ++round) {
    if (tid < 2) s_count[tid] = 0;                // [0] unmatched targets of this round, [1] rows holding more than one target
    __syncthreads();
    for (int g = wv; g < G; g += kWaves) {        // targets without a query
      bool any = false;
      if (exists(g))
        for (int q = lane; q < Q; q += 64) any = any || (M[(int64_t)q * G + g] & kMatch);
      const bool un = exists(g) && __ballot(any) == 0ull;
      if (lane == 0) {
        s_unmatched[g] = un ? 1 : 0;
        if (un) atomicAdd(&s_count[0], 1);
      }
    }
    __syncthreads();
    if (s_count[0] == 0) break;
    if (round >= max_rounds) { st = 2; break; }
    for (int q = tid; q < Q; q += kThreads) {     // cost[matched_query_id] += 100000.0
      if (row_sum(q) > 0)
        for (int g = 0; g < G; ++g) C[(int64_t)q * G + g] = C[(int64_t)q * G + g] + kTakenPenalty;
    }
    __syncthreads();
    for (int g = wv; g < G; g += kWaves) {        // every unmatched target takes its cheapest query (torch.argmin: first minimum)
      if (!s_unmatched[g]) continue;
      float bv = INFINITY;
      int bi = 0x7fffffff;
      for (int q = lane; q < Q; q += 64) {
        const float v = nan_first(C[(int64_t)q * G + g]);
        if (v < bv || (v == bv && q < bi)) { bv = v; bi = q; }
      }
      wave_ops::wave_argmin(bv, bi);
      if (lane == 0 && bi != 0x7fffffff) M[(int64_t)bi * G + g] |= kMatch;
    }
    __syncthreads();
    for (int q = tid; q < Q; q += kThreads)
      if (row_sum(q) > 1) atomicAdd(&s_count[1], 1);
    __syncthreads();
    if (s_count[1] > 0) {
      // the reference indexes with the mask computed BEFORE the loop (`anchor_matching_gt > 1`, never refreshed): those rows,
      // and only those, are reset to their cheapest target -- whether or not they are the rows in conflict now
      for (int q = tid; q < Q; q += kThreads)
        if (M[(int64_t)q * G] & kStale) keep_cheapest(q);
    }
    __syncthreads();
  }
  __syncthreads();
  for (int q = tid; q < Q; q += kThreads) M[(int64_t)q * G] &= kMatch;     // the result is the 0 / 1 matrix
  __syncthreads();
  return st;
}

// ---- host: image b owns elements off[b] .. off[b + 1] - 1 of a concatenated array; passed to the kernels by value ------------
struct BatchOffsets { int32_t off[OTA_HIP_MAX_BATCH + 1]; };

// Checks and copies a host offset array (gt_off, or the re-ID loss's item_off); *max_g: the largest image.  min_batch: 0 where an
// empty batch is a valid call (it then needs no array), 1 where it is refused.
inline int fill_offsets(const int32_t* host_off, int batch, int min_batch, BatchOffsets* go, int* max_g) {
  if (batch < min_batch || batch > OTA_HIP_MAX_BATCH)
    return set_error(OTA_ERR_BAD_DIMS, min_batch ? "reid: batch out of range (1 .. OTA_HIP_MAX_BATCH)" : "ota: batch out of range (<= OTA_HIP_MAX_BATCH)");
  if (batch > 0 && !host_off) return set_error(OTA_ERR_NULL_POINTER, "ota: gt_off is null");
  *max_g = 0;
  for (int b = 0; b <= batch; ++b) go->off[b] = batch ? host_off[b] : 0;
  if (go->off[0] != 0) return set_error(OTA_ERR_BAD_DIMS, "ota: gt_off[0] must be 0");
  for (int b = 0; b < batch; ++b) {
    const int g = go->off[b + 1] - go->off[b];
    if (g < 0) return set_error(OTA_ERR_BAD_DIMS, "ota: gt_off must be non-decreasing");
    if (g > *max_g) *max_g = g;
  }
  return 0;
}

}  // namespace msda
