// The online IDOL tracker's association and memory bank (models/tracker.py:98-298) -- see include/dynmask_hip.h (track_hip_*).
//
//   memo_embed   one workgroup per live slot: the score-weighted mean of its ring, oldest to newest (long_match only).
//   feats_rows   one workgroup per kept detection: a wave forms one dot product at a time (16-byte loads when D is a multiple
//                of 4), the row stays in LDS for its maximum and its sum of exponentials.
//   cols_final   one lane per memory column: the column's maximum and sum over the kept rows, then the bi-softmax scores.
//   associate    ONE workgroup: walks the kept detections in order (row maximum with the lowest-index tie rule, the
//                frame_weight branch, column zeroing kept as a `taken` table in LDS), numbers the new tracklets, runs the
//                backdrop test on the pre-NMS' inter / area, and plans the update: which row feeds which slot, and where every
//                surviving slot and every new tracklet lands after the stable compaction.
//   update       one workgroup per old slot and per detection: writes the NEXT state out of place, so no slot is read after it
//                has been overwritten.
//
// The layout helpers, the bi-softmax of feats_rows / cols_final and the update of the common fields: track_bank.hpp.
// Every barrier sits in control flow that is uniform over the workgroup.  Compiled without contraction; no atomics; every
// reduction in a fixed order: bitwise repeatable.
#pragma clang fp contract(off)
#include "../../include/dynmask_hip.h"

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "track_bank.hpp"

namespace track {

using bank::kBox, bank::kMaxC, bank::kMaxN, bank::kThreads, bank::kWaves;
constexpr int kMaxL = TRACK_HIP_MAX_MEMORY_LEN;
static_assert(kMaxC * 4 + kMaxN * 10 + 256 <= 64 * 1024, "associate stays under the LDS a launch gets without opting in");

struct State : bank::Slots {      // meta [2]: count, num_tracklets
  int* exist_frame;     // [C]
  int* long_len;        // [C]
  float* long_score;    // [C, L]
  float* long_embed;    // [C, L, D]
};

// the fields' sizes in the order of the bank (include/dynmask_hip.h) for capacity C, width D, ring length L
struct Sizes {
  size_t of[TRACK_HIP_STATE_FIELDS];
  size_t offset(int field) const { return bank::offset(of, TRACK_HIP_STATE_FIELDS, field); }
};

inline Sizes sizes(size_t C, size_t D, size_t L) {
  return {{16, 8 * C, 8 * C, 4 * kBox * C, 4 * kBox * C, 4 * C, 4 * C, 4 * C, 4 * C, 4 * C * L, 4 * C * D, 4 * C * L * D}};
}

inline State view(const void* base, int C, int D, int L) {
  const Sizes z = sizes(C, D, L);
  State s;
  bank::view_slots(&s, base, z.of, TRACK_HIP_STATE_FIELDS, 10);
  s.exist_frame = bank::at<int>(base, z.offset(7));
  s.long_len = bank::at<int>(base, z.offset(8));
  s.long_score = bank::at<float>(base, z.offset(9));
  s.long_embed = bank::at<float>(base, z.offset(11));
  return s;
}

__global__ void __launch_bounds__(kThreads)
memo_embed(State s, const float* __restrict__ temporal, int D, int L, float* __restrict__ out) {
  const int m = blockIdx.x;
  const int len = min(max(s.long_len[m], 0), L);
  const float* __restrict__ score = s.long_score + (size_t)m * L;
  const float* __restrict__ tw = temporal ? temporal + (size_t)len * L : nullptr;      // row `length` of the table
  float wsum = 0.f;
  for (int k = 0; k < len; ++k) wsum += tw ? score[k] + tw[k] : score[k];
  const float* __restrict__ ring = s.long_embed + (size_t)m * L * D;
  for (int d = threadIdx.x; d < D; d += kThreads) {
    float acc = 0.f;
    for (int k = 0; k < len; ++k) acc += ring[(size_t)k * D + d] * (tw ? score[k] + tw[k] : score[k]);
    out[(size_t)m * D + d] = __fdiv_rn(acc, wsum);
  }
}

__global__ void __launch_bounds__(kThreads)
feats_rows(const float* __restrict__ embeds, const unsigned char* __restrict__ keep, const float* __restrict__ memo, int M, int D,
           int vec, float* __restrict__ feats, float* __restrict__ rstat) {
  const int i = blockIdx.x;
  if (!keep[i]) return;                        // uniform over the workgroup, before the first barrier
  bank::score_row<kMaxC>(embeds + (size_t)i * D, [=](int m) { return memo + (size_t)m * D; }, i, M, D, vec, feats, rstat);
}

__global__ void __launch_bounds__(kThreads)
cols_final(const unsigned char* __restrict__ keep, const float* __restrict__ rstat, int n, int M, float* __restrict__ scores) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;                          // no barrier in this kernel
  bank::col_softmax(keep, rstat, n, M, m, scores);
}

__device__ __forceinline__ float mask_iou(const int* __restrict__ inter, const int* __restrict__ area, int n, int i, int j) {
  const int it = inter[(size_t)i * n + j], un = area[i] + area[j] - it;
  return __fdiv_rn(__fadd_rn((float)it, 1e-6f), __fadd_rn((float)un, 1e-6f));
}

__global__ void __launch_bounds__(kThreads)
associate(const float* __restrict__ scores, const unsigned char* __restrict__ keep, const float* __restrict__ bboxes,
          const int* __restrict__ inter, const int* __restrict__ area, State s, long long* __restrict__ next_meta, int n, int M,
          int capacity, int frame_weight, float match_thr, float new_thr, float nms_thr_post, int frame_id, int tracklet_frames,
          int* __restrict__ plan, long long* __restrict__ out) {
  __shared__ int taken[kMaxC];                 // row + 1 of the detection that took the column, 0: free
  __shared__ long long ids[kMaxN];
  __shared__ unsigned char kept[kMaxN];
  __shared__ unsigned char fresh[kMaxN];       // the detection starts a tracklet
  __shared__ float wbest[kWaves];
  __shared__ int wind[kWaves], wcnt[kWaves], wexist[kWaves];
  __shared__ long long totals[2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

  for (int m = tid; m < M; m += kThreads) taken[m] = 0;
  for (int i = tid; i < n; i += kThreads) {
    ids[i] = -2;
    kept[i] = keep[i] ? 1 : 0;
    fresh[i] = 0;
  }
  __syncthreads();

  // tracker.py:245-264.  n, M, kept[i] and frame_weight are the same for every thread: every barrier below is uniform.
  if (M > 0) {
    for (int i = 0; i < n; ++i) {
      if (!kept[i]) continue;
      const float* __restrict__ srow = scores + (size_t)i * M;
      bool weighted = false;
      float mean = 0.f;
      if (frame_weight) {
        int cnt = 0, exist = 0;
        for (int m = tid; m < M; m += kThreads) {
          const float v = taken[m] ? 0.f : srow[m];
          if (v > 0.5f) {
            ++cnt;
            exist += s.exist_frame[m];
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {     // (written out: two wave_sum calls change this kernel's assembly)
          cnt += __shfl_xor(cnt, o, 64);
          exist += __shfl_xor(exist, o, 64);
        }
        if (lane == 0) {
          wcnt[wv] = cnt;
          wexist[wv] = exist;
        }
        __syncthreads();
        cnt = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        exist = wexist[0] + wexist[1] + wexist[2] + wexist[3];
        weighted = cnt > 1;
        if (weighted) mean = __fdiv_rn((float)exist, (float)cnt);
      }
      float best = -INFINITY;
      int bi = INT_MAX;
      for (int m = tid; m < M; m += kThreads) {
        float v = taken[m] ? 0.f : srow[m];
        if (weighted) v = v > 0.5f ? v * (float)s.exist_frame[m] : v * mean;
        if (v > best) {
          best = v;
          bi = m;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {       // (written out: wave_ops::wave_argmax changes this kernel's assembly)
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) {
          best = ov;
          bi = oi;
        }
      }
      if (lane == 0) {
        wbest[wv] = best;
        wind[wv] = bi;
      }
      __syncthreads();
      best = wbest[0];
      bi = wind[0];
#pragma unroll
      for (int k = 1; k < kWaves; ++k)
        if (wbest[k] > best || (wbest[k] == best && wind[k] < bi)) {
          best = wbest[k];
          bi = wind[k];
        }
      if (tid == 0 && bi < M && best > match_thr) {
        ids[i] = s.id[bi];
        taken[bi] = i + 1;
      }
      __syncthreads();                         // the column is taken, and the partial results may be overwritten
    }
  }

  // tracker.py:265-271 / :282-288: new tracklets in detection order
  if (wv == 0) {
    long long next = s.meta[1];
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const bool is_new = i < n && kept[i] && ids[i] == -2 && bboxes[(size_t)i * kBox + 4] > new_thr;
      const unsigned long long mask = __ballot(is_new);
      if (is_new) {
        ids[i] = next + __popcll(mask & ((1ull << lane) - 1ull));
        fresh[i] = 1;
      }
      next += __popcll(mask);
    }
    if (lane == 0) totals[1] = next;
  }
  __syncthreads();

  // tracker.py:273-277: an unselected detection whose mask stays below nms_thr_post with every earlier kept one is a backdrop
  for (int i = wv; i < n; i += kWaves) {       // wave-uniform; no workgroup barrier inside
    if (!kept[i] || ids[i] != -2) continue;
    bool overlaps = false;
    for (int j = lane; j < i; j += 64)
      if (kept[j] && !(mask_iou(inter, area, n, i, j) < nms_thr_post)) overlaps = true;
    if (!__any(overlaps) && lane == 0) ids[i] = -1;
  }
  __syncthreads();

  // the update's plan: plan[0 .. capacity) the row that feeds a slot (-1: none), plan[capacity .. 2 capacity) where the slot
  // lands (-1: it expires, tracker.py:152-161), plan[2 capacity .. + n) where a detection's new tracklet lands (-1: none)
  if (wv == 0) {
    int count = 0;
    for (int base = 0; base < M; base += 64) {
      const int m = base + lane;
      const int row = m < M ? taken[m] - 1 : -1;
      const bool alive = m < M && frame_id - (row >= 0 ? frame_id : s.last_frame[m]) < tracklet_frames;
      const unsigned long long mask = __ballot(alive);
      if (m < M) {
        plan[m] = row;
        plan[capacity + m] = alive ? count + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
      }
      count += __popcll(mask);
    }
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const bool alive = i < n && fresh[i] && 0 < tracklet_frames;
      const unsigned long long mask = __ballot(alive);
      const int dst = count + __popcll(mask & ((1ull << lane) - 1ull));
      if (i < n) plan[2 * capacity + i] = alive && dst < capacity ? dst : -1;
      count += __popcll(mask);
    }
    if (lane == 0) totals[0] = min(count, capacity);
  }
  __syncthreads();
  for (int i = tid; i < n; i += kThreads) {
    out[i] = kept[i];
    out[n + i] = kept[i] ? ids[i] : -3;
  }
  if (wv == 0) {                               // the kept rows in order, for the caller's gathers
    int count = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const bool on = i < n && kept[i];
      const unsigned long long mask = __ballot(on);
      if (on) out[2 * n + 2 + count + __popcll(mask & ((1ull << lane) - 1ull))] = i;
      count += __popcll(mask);
    }
    for (int i = count + lane; i < n; i += 64) out[2 * n + 2 + i] = 0;
  }
  if (tid == 0) {
    out[2 * n] = totals[0];
    out[2 * n + 1] = totals[1];
    next_meta[0] = totals[0];
    next_meta[1] = totals[1];
  }
}

__global__ void __launch_bounds__(kThreads)
update(const float* __restrict__ embeds, const float* __restrict__ bboxes, const long long* __restrict__ labels,
       const int* __restrict__ plan, const long long* __restrict__ result, State a, State b, int n, int M, int capacity, int D, int L, float keep_weight,
       float momentum, int frame_id) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= M) {                  // tracker.py:132-141: a new tracklet
    const int i = blockIdx.x - M, dst = plan[2 * capacity + i];
    if (dst < 0) return;
    const float* __restrict__ e = embeds + (size_t)i * D;
    bank::slot_new<true>(b, dst, D, e, b.long_embed + (size_t)dst * L * D, bboxes + (size_t)i * kBox, result[n + i], labels[i], frame_id);
    if (tid == 0) {
      b.long_score[(size_t)dst * L] = bboxes[(size_t)i * kBox + 4];
      b.exist_frame[dst] = 1;
      b.long_len[dst] = 1;
    }
    return;
  }
  const int m = blockIdx.x, dst = plan[capacity + m], row = plan[m];
  if (dst < 0) return;
  const int len = min(max(a.long_len[m], 0), L);
  const float* __restrict__ ring = a.long_embed + (size_t)m * L * D;
  float* __restrict__ ring_out = b.long_embed + (size_t)dst * L * D;
  const float* __restrict__ score = a.long_score + (size_t)m * L;
  float* __restrict__ score_out = b.long_score + (size_t)dst * L;
  if (row < 0) {                               // not seen in this frame: the slot moves as it is
    bank::slot_move(a, b, dst, m, D);
    for (int k = tid; k < len * D; k += kThreads) ring_out[k] = ring[k];
    for (int k = tid; k < len; k += kThreads) score_out[k] = score[k];
    if (tid == 0) {
      b.exist_frame[dst] = a.exist_frame[m];
      b.long_len[dst] = len;
    }
    return;
  }
  // tracker.py:111-129; the oldest ring entry leaves when the ring is full (:156-159)
  const float* __restrict__ e = embeds + (size_t)row * D;
  const int drop = len == L ? 1 : 0, kept_len = len - drop;
  bank::slot_match<true>(a, b, dst, m, D, e, ring_out + (size_t)kept_len * D, bboxes + (size_t)row * kBox, labels[row], keep_weight, momentum,
                   frame_id);
  for (int k = tid; k < kept_len * D; k += kThreads) ring_out[k] = ring[k + drop * D];
  for (int k = tid; k < kept_len; k += kThreads) score_out[k] = score[k + drop];
  if (tid == 0) {
    score_out[kept_len] = bboxes[(size_t)row * kBox + 4];
    b.exist_frame[dst] = a.exist_frame[m] + 1;
    b.long_len[dst] = kept_len + 1;
  }
}

inline bool geometry_ok(int n, int M, int capacity, int D, int L) { return bank::geometry_ok(n, M, capacity, D) && L >= 1; }

inline bool sizes_ok(int n, int capacity, int D, int L) { return bank::sizes_ok(n, capacity, D) && L <= kMaxL; }

}  // namespace track

extern "C" {

static const char* g_track_last = "";

const char* track_hip_last_kernel(void) { return g_track_last; }

size_t track_hip_state_offset(int field, int capacity, int D, int memory_len) {
  if (field < 0 || field > TRACK_HIP_STATE_FIELDS || capacity < 1 || D < 1 || memory_len < 1) return 0;
  return track::sizes(capacity, D, memory_len).offset(field);
}

int track_hip_scores_f32(const float* embeds, const unsigned char* keep, const void* state, const float* temporal, int long_match,
                         int n, int M, int capacity, int D, int memory_len, float* memo_embed, float* row_stats, float* scores,
                         void* stream) {
  using namespace track;
  if (!geometry_ok(n, M, capacity, D, memory_len)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "track_scores: bad dimensions");
  if (!sizes_ok(n, capacity, D, memory_len))
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "track_scores: at most 1024 detections, 4096 slots, width 256, ring 64");
  if (n == 0 || M == 0) return 0;
  if (!embeds || !keep || !state || !row_stats || !scores || (long_match && !memo_embed))
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "track_scores: null pointer argument");
  const State s = view(state, capacity, D, memory_len);
  const float* memo = s.embed;
  if (long_match) {
    hipLaunchKernelGGL(track::memo_embed, dim3((unsigned)M), dim3(kThreads), 0, (hipStream_t)stream, s, temporal, D, memory_len,
                       memo_embed);
    memo = memo_embed;
  }
  const int vec = bank::vec_rows(D, {embeds, memo});
  hipLaunchKernelGGL(feats_rows, dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, embeds, keep, memo, M, D, vec, scores,
                     row_stats);
  hipLaunchKernelGGL(cols_final, dim3((unsigned)msda::ceil_div(M, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, keep, row_stats,
                     n, M, scores);
  if (const int e = msda::launch_status()) return e;
  g_track_last = long_match ? "track_scores<long>" : "track_scores";
  return 0;
}

int track_hip_associate_f32(const float* scores, const unsigned char* keep, const float* bboxes, const int* inter, const int* area,
                            const void* state, void* next_state, int n, int M, int capacity, int D, int memory_len, int frame_weight,
                            float match_score_thr, float new_score_thr, float nms_thr_post, int frame_id, int memo_tracklet_frames,
                            int* plan, long long* result, void* stream) {
  using namespace track;
  if (!geometry_ok(n, M, capacity, D, memory_len) || !bank::fits(n, M, capacity))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "track_associate: bad dimensions (M + n must fit the capacity)");
  if (!sizes_ok(n, capacity, D, memory_len))
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "track_associate: at most 1024 detections, 4096 slots, width 256, ring 64");
  if (n == 0) return 0;
  if (!keep || !bboxes || !inter || !area || !state || !next_state || !plan || !result || (M > 0 && !scores))
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "track_associate: null pointer argument");
  const State s = view(state, capacity, D, memory_len), t = view(next_state, capacity, D, memory_len);
  hipLaunchKernelGGL(associate, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, scores, keep, bboxes, inter, area, s, t.meta, n, M,
                     capacity, frame_weight ? 1 : 0, match_score_thr, new_score_thr, nms_thr_post, frame_id, memo_tracklet_frames, plan,
                     result);
  if (const int e = msda::launch_status()) return e;
  g_track_last = "track_associate";
  return 0;
}

int track_hip_update_f32(const float* embeds, const float* bboxes, const long long* labels, const int* plan, const long long* result,
                         const void* state, void* next_state, int n, int M, int capacity, int D, int memory_len, float keep_weight,
                         float momentum, int frame_id, void* stream) {
  using namespace track;
  if (!geometry_ok(n, M, capacity, D, memory_len) || !bank::fits(n, M, capacity))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "track_update: bad dimensions (M + n must fit the capacity)");
  if (!sizes_ok(n, capacity, D, memory_len))
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "track_update: at most 1024 detections, 4096 slots, width 256, ring 64");
  if (state == next_state) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "track_update: the next state must be another buffer");
  if (n == 0) return 0;
  if (!embeds || !bboxes || !labels || !plan || !result || !state || !next_state)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "track_update: null pointer argument");
  const State a = view(state, capacity, D, memory_len), b = view(next_state, capacity, D, memory_len);
  hipLaunchKernelGGL(update, dim3((unsigned)(M + n)), dim3(kThreads), 0, (hipStream_t)stream, embeds, bboxes, labels, plan, result, a, b,
                     n, M, capacity, D, memory_len, keep_weight, momentum, frame_id);
  if (const int e = msda::launch_status()) return e;
  g_track_last = "track_update";
  return 0;
}

}  // extern "C"
