// The QuasiDense embedding tracker's box pre-NMS, association and memory bank (models/tracker.py:304-503, the bdd_track
// route; util/mmcv_utils.py:146-191 for the box IoU) -- see include/dynmask_hip.h (qdtrack_hip_*).
//
//   rank         one lane per detection: its place in the descending order of the scores, by counting (equal scores: the lower
//                index first), written as order[place] = detection.
//   iou_valid    one wave per sorted row: the row of the box IoU matrix, and whether any EARLIER sorted row lies above the row's
//                threshold.  Not a greedy NMS: a dropped row still drops later ones, so the rows are independent.
//   feats_rows   one workgroup per valid row: a wave forms one dot product at a time against the memory's columns (the live
//                tracklets, then the backdrop frames newest first); the row stays in LDS for its maximum and its sum.
//   cols_final   one lane per memory column: the column's maximum and sum over the valid rows, the bi-softmax score and the
//                class gate.
//   associate    ONE workgroup: walks the valid rows in order (row maximum with the lowest-index tie rule, taken tracklet
//                columns read as 0, the three outcomes id / -2 / -1), numbers the new tracklets, filters the new backdrop frame
//                on the box IoU, compacts the valid rows and plans the update.
//   update       one workgroup per old slot, per sorted row and per backdrop row that moves down the ring: writes the NEXT
//                state out of place.
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
#include "wave_ops.hpp"

namespace qdtrack {

using wave_ops::wave_argmax;
using bank::kBox, bank::kMaxC, bank::kMaxN, bank::kThreads, bank::kWaves;
constexpr int kMaxB = QDTRACK_HIP_MAX_BACKDROPS;
constexpr int kMaxK = QDTRACK_HIP_MAX_BACKDROP_FRAMES;
constexpr int kMaxCols = kMaxC + kMaxK * kMaxB;
constexpr int kMeta = 2 + kMaxK;
static_assert(kMaxCols * 4 + 256 <= 64 * 1024, "feats_rows stays under the LDS a launch gets without opting in");
static_assert(kMaxC * 4 + kMaxN * 11 + 256 <= 64 * 1024, "so does associate");

struct State : bank::Slots {      // meta [2 + kMaxK]: count, num_tracklets, the rows of backdrop frame 0 (the newest), 1, ...
  long long* bd_label;  // [K, B]
  float* bd_bbox;       // [K, B, 5]
  float* bd_embed;      // [K, B, D]
};

// the memory's columns: M live tracklets, then cnt[k] rows of backdrop frame k for k < K
struct Cols {
  int M, K, total;
  int cnt[kMaxK];
};

// the fields' sizes in the order of the bank (include/dynmask_hip.h) for capacity C, width D, B backdrops in each of `frames`
// frames (a ring of one when there are none)
struct Sizes {
  size_t of[QDTRACK_HIP_STATE_FIELDS];
  size_t offset(int field) const { return bank::offset(of, QDTRACK_HIP_STATE_FIELDS, field); }
};

inline Sizes sizes(size_t C, size_t D, size_t B, int frames) {
  const size_t KB = B * (frames > 0 ? frames : 1);
  return {{8 * kMeta, 8 * C, 8 * C, 4 * kBox * C, 4 * kBox * C, 4 * C, 4 * C, 4 * C * D, 8 * KB, 4 * kBox * KB, 4 * KB * D}};
}

inline State view(const void* base, int C, int D, int B, int frames) {
  const Sizes z = sizes(C, D, B, frames);
  State s;
  bank::view_slots(&s, base, z.of, QDTRACK_HIP_STATE_FIELDS, 7);
  s.bd_label = bank::at<long long>(base, z.offset(8));
  s.bd_bbox = bank::at<float>(base, z.offset(9));
  s.bd_embed = bank::at<float>(base, z.offset(10));
  return s;
}

// the row of bd_* that memory column m >= M stands for (frame * B + row), -1 past the last column
__device__ __forceinline__ int backdrop_row(const Cols& c, int m, int B) {
  int off = m - c.M;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    if (k < c.K) {
      if (off < c.cnt[k]) return k * B + off;
      off -= c.cnt[k];
    }
  }
  return -1;
}

// a key whose unsigned order is the order of the floats (-0.0 as +0.0), total even for values that are no numbers
__device__ __forceinline__ unsigned score_key(float f) {
  if (f == 0.f) f = 0.f;
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(kThreads)
rank(const float* __restrict__ bboxes, int n, int* __restrict__ order) {
  __shared__ unsigned key[kMaxN];
  for (int j = threadIdx.x; j < n; j += kThreads) key[j] = score_key(bboxes[(size_t)j * kBox + 4]);
  __syncthreads();
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;                          // after the only barrier
  const unsigned mine = key[i];
  int place = 0;
  for (int j = 0; j < n; ++j) place += (key[j] > mine || (key[j] == mine && j < i)) ? 1 : 0;
  order[place] = i;                            // a total order: `place` is a permutation of [0, n)
}

// mmcv_utils.py:149-189, mode 'iou', not aligned, eps 1e-6: one IEEE operation per operation of the reference
__device__ __forceinline__ float box_iou(float ax1, float ay1, float ax2, float ay2, float area_a, const float* __restrict__ b) {
  const float bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
  const float area_b = (bx2 - bx1) * (by2 - by1);
  const float w = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f);
  const float h = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
  const float overlap = w * h;
  const float uni = fmaxf(area_a + area_b - overlap, 1e-6f);
  return __fdiv_rn(overlap, uni);
}

__global__ void __launch_bounds__(kThreads)
iou_valid(const float* __restrict__ bboxes, const int* __restrict__ order, int n, float obj_thr, float backdrop_thr, float class_thr,
          float* __restrict__ iou, unsigned char* __restrict__ valid) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= n) return;                          // wave-uniform; no barrier in this kernel
  const float* __restrict__ a = bboxes + (size_t)order[i] * kBox;
  const float ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3];
  const float area_a = (ax2 - ax1) * (ay2 - ay1);
  const float thr = a[4] < obj_thr ? backdrop_thr : class_thr;      // tracker.py:443-444
  bool hit = false;
  for (int j = lane; j < n; j += 64) {
    const float v = box_iou(ax1, ay1, ax2, ay2, area_a, bboxes + (size_t)order[j] * kBox);
    iou[(size_t)i * n + j] = v;
    if (j < i && v > thr) hit = true;
  }
  hit = __any(hit);
  if (lane == 0) valid[i] = hit ? 0 : 1;
}

__global__ void __launch_bounds__(kThreads)
feats_rows(const float* __restrict__ embeds, const int* __restrict__ order, const unsigned char* __restrict__ valid, State s, Cols c,
           int D, int B, int vec, float* __restrict__ feats, float* __restrict__ rstat) {
  const int i = blockIdx.x;
  if (!valid[i]) return;                       // uniform over the workgroup, before the first barrier
  auto col = [&](int m) { return m < c.M ? s.embed + (size_t)m * D : s.bd_embed + (size_t)max(backdrop_row(c, m, B), 0) * D; };
  bank::score_row<kMaxCols>(embeds + (size_t)order[i] * D, col, i, c.total, D, vec, feats, rstat);
}

__global__ void __launch_bounds__(kThreads)
cols_final(const long long* __restrict__ labels, const int* __restrict__ order, const unsigned char* __restrict__ valid,
           const float* __restrict__ rstat, State s, Cols c, int n, int B, int with_cats, float* __restrict__ scores) {
  const int m = blockIdx.x * kThreads + threadIdx.x, Mt = c.total;
  if (m >= Mt) return;                         // no barrier in this kernel
  bank::col_softmax(valid, rstat, n, Mt, m, scores, [&] {      // tracker.py:477-479: the class gate
    const long long mine = m < c.M ? s.label[m] : s.bd_label[max(backdrop_row(c, m, B), 0)];
    return [=](int i, float v) {
      if (with_cats) v *= labels[order[i]] == mine ? 1.f : 0.f;
      return v;
    };
  });
}

__global__ void __launch_bounds__(kThreads)
associate(const float* __restrict__ scores, const unsigned char* __restrict__ valid, const int* __restrict__ order,
          const float* __restrict__ bboxes, const float* __restrict__ iou, State s, Cols c, long long* __restrict__ next_meta, int n,
          int capacity, int B, float match_thr, float obj_thr, float conf_thr, float init_thr, float backdrop_thr, int frame_id,
          int tracklet_frames, int* __restrict__ plan, long long* __restrict__ out) {
  __shared__ int taken[kMaxC];                 // sorted row + 1 of the detection that took the tracklet's column, 0: free
  __shared__ long long ids[kMaxN];
  __shared__ unsigned char val[kMaxN];
  __shared__ unsigned char fresh[kMaxN];       // the row starts a tracklet
  __shared__ unsigned char backdrop[kMaxN];    // the row goes into the new backdrop frame
  __shared__ float wbest[kWaves];
  __shared__ int wind[kWaves];
  __shared__ long long totals[4];              // valid rows, next count, next num_tracklets, rows of the new backdrop frame
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, M = c.M, Mt = c.total;

  for (int m = tid; m < M; m += kThreads) taken[m] = 0;
  for (int i = tid; i < n; i += kThreads) {
    ids[i] = -1;
    val[i] = valid[i] ? 1 : 0;
    fresh[i] = 0;
    backdrop[i] = 0;
  }
  __syncthreads();

  // tracker.py:458-492.  n, M, Mt and val[i] are the same for every thread: every barrier below is uniform.
  if (M > 0) {
    for (int i = 0; i < n; ++i) {
      if (!val[i]) continue;
      const float* __restrict__ srow = scores + (size_t)i * Mt;
      float best = -INFINITY;
      int bi = INT_MAX;
      for (int m = tid; m < Mt; m += kThreads) {
        const float v = (m < M && taken[m]) ? 0.f : srow[m];
        if (v > best) {
          best = v;
          bi = m;
        }
      }
      wave_argmax(best, bi);
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
      if (tid == 0 && bi < M && best > match_thr) {      // a best column that is a backdrop (bi >= M) changes nothing
        if (bboxes[(size_t)order[i] * kBox + 4] > obj_thr) {
          ids[i] = s.id[bi];
          taken[bi] = i + 1;
        } else if (best > conf_thr) {
          ids[i] = -2;
        }
      }
      __syncthreads();                         // the column is taken, and the partial results may be overwritten
    }
  }

  // tracker.py:493-499: new tracklets in row order
  if (wv == 0) {
    long long next = s.meta[1];
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const bool is_new = i < n && val[i] && ids[i] == -1 && bboxes[(size_t)order[i] * kBox + 4] > init_thr;
      const unsigned long long mask = __ballot(is_new);
      if (is_new) {
        ids[i] = next + __popcll(mask & ((1ull << lane) - 1ull));
        fresh[i] = 1;
      }
      next += __popcll(mask);
    }
    if (lane == 0) totals[2] = next;
  }
  __syncthreads();

  // tracker.py:374-379: a row still -1 is a backdrop unless its box overlaps an earlier valid row's above nms_backdrop_iou_thr
  for (int i = wv; i < n; i += kWaves) {       // wave-uniform; no workgroup barrier inside
    if (!val[i] || ids[i] != -1) continue;
    bool overlaps = false;
    for (int j = lane; j < i; j += 64)
      if (val[j] && iou[(size_t)i * n + j] > backdrop_thr) overlaps = true;
    if (!__any(overlaps) && lane == 0) backdrop[i] = 1;
  }
  __syncthreads();

  // the update's plan: plan[0 .. capacity) the detection that feeds a slot (-1: none), plan[capacity .. 2 capacity) where the
  // slot lands (-1: it expires, tracker.py:389-394), plan[2 capacity .. + n) where a sorted row's new tracklet lands and
  // plan[2 capacity + n .. + 2 n) its row of the new backdrop frame (-1: none)
  if (wv == 0) {
    int count = 0;
    for (int base = 0; base < M; base += 64) {
      const int m = base + lane;
      const int row = m < M ? taken[m] - 1 : -1;
      const bool alive = m < M && frame_id - (row >= 0 ? frame_id : s.last_frame[m]) < tracklet_frames;
      const unsigned long long mask = __ballot(alive);
      if (m < M) {
        plan[m] = row >= 0 ? order[row] : -1;
        plan[capacity + m] = alive ? count + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
      }
      count += __popcll(mask);
    }
    int drops = 0, rows = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const bool alive = i < n && fresh[i] && 0 < tracklet_frames;
      const unsigned long long mask = __ballot(alive);
      const int dst = count + __popcll(mask & ((1ull << lane) - 1ull));
      if (i < n) plan[2 * capacity + i] = alive && dst < capacity ? dst : -1;
      count += __popcll(mask);
      const bool drop = i < n && backdrop[i] && c.K > 0;
      const unsigned long long dmask = __ballot(drop);
      const int ddst = drops + __popcll(dmask & ((1ull << lane) - 1ull));
      if (i < n) plan[2 * capacity + n + i] = drop && ddst < B ? ddst : -1;
      drops += __popcll(dmask);
      // the valid rows in order: their detections (for the caller's gathers), their ids and their sorted rows
      const bool on = i < n && val[i];
      const unsigned long long vmask = __ballot(on);
      if (on) {
        const int p = rows + __popcll(vmask & ((1ull << lane) - 1ull));
        out[p] = order[i];
        out[n + p] = ids[i];
        out[2 * n + p] = i;
      }
      rows += __popcll(vmask);
    }
    for (int p = rows + lane; p < n; p += 64) {
      out[p] = 0;
      out[n + p] = -3;
      out[2 * n + p] = 0;
    }
    if (lane == 0) {
      totals[0] = rows;
      totals[1] = min(count, capacity);
      totals[3] = min(drops, B);
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += kThreads) out[3 * n + 4 + i] = val[i] ? ids[i] : -3;      // by sorted row, for the update
  if (tid == 0) {
    out[3 * n] = totals[0];
    out[3 * n + 1] = totals[1];
    out[3 * n + 2] = totals[2];
    out[3 * n + 3] = totals[3];
    next_meta[0] = totals[1];
    next_meta[1] = totals[2];
    next_meta[2] = totals[3];
#pragma unroll
    for (int k = 1; k < kMaxK; ++k) next_meta[2 + k] = k < c.K ? c.cnt[k - 1] : 0;
  }
}

__global__ void __launch_bounds__(kThreads)
update(const float* __restrict__ embeds, const float* __restrict__ bboxes, const long long* __restrict__ labels,
       const int* __restrict__ order, const int* __restrict__ plan, const long long* __restrict__ result, State a, State b, Cols c, int n,
       int capacity, int D, int B, float keep_weight, float momentum, int frame_id) {
  const int tid = threadIdx.x, M = c.M;
  int blk = blockIdx.x;
  if (blk >= M + n) {                          // tracker.py:381, :396-397: an older backdrop frame moves one place down the ring
    int r = blk - M - n, from = -1;
#pragma unroll
    for (int k = 0; k + 1 < kMaxK; ++k) {
      if (k + 1 < c.K && from < 0) {
        if (r < c.cnt[k]) from = k * B + r;
        else r -= c.cnt[k];
      }
    }
    if (from < 0) return;
    const int to = from + B;
    for (int d = tid; d < D; d += kThreads) b.bd_embed[(size_t)to * D + d] = a.bd_embed[(size_t)from * D + d];
    if (tid < kBox) b.bd_bbox[to * kBox + tid] = a.bd_bbox[from * kBox + tid];
    if (tid == 0) b.bd_label[to] = a.bd_label[from];
    return;
  }
  if (blk >= M) {                              // a sorted row: a new tracklet (tracker.py:366-372), a backdrop, or neither
    const int i = blk - M, src = order[i], dst = plan[2 * capacity + i], drop = plan[2 * capacity + n + i];
    const float* __restrict__ e = embeds + (size_t)src * D;
    if (dst >= 0) {
      bank::slot_new<false>(b, dst, D, e, nullptr, bboxes + (size_t)src * kBox, result[3 * n + 4 + i], labels[src], frame_id);
    } else if (drop >= 0) {
      for (int d = tid; d < D; d += kThreads) b.bd_embed[(size_t)drop * D + d] = e[d];
      if (tid < kBox) b.bd_bbox[drop * kBox + tid] = bboxes[(size_t)src * kBox + tid];
      if (tid == 0) b.bd_label[drop] = labels[src];
    }
    return;
  }
  const int m = blk, dst = plan[capacity + m], row = plan[m];
  if (dst < 0) return;
  if (row < 0) bank::slot_move(a, b, dst, m, D);      // not seen in this frame: the slot moves as it is
  else bank::slot_match<false>(a, b, dst, m, D, embeds + (size_t)row * D, nullptr, bboxes + (size_t)row * kBox, labels[row], keep_weight,
                        momentum, frame_id);          // tracker.py:351-364
}

inline bool geometry_ok(int n, int M, int capacity, int D, int B, int frames) {
  return bank::geometry_ok(n, M, capacity, D) && B >= 1 && frames >= 0;
}

inline bool sizes_ok(int n, int capacity, int D, int B, int frames) { return bank::sizes_ok(n, capacity, D) && B <= kMaxB && frames <= kMaxK; }

// the memory's columns from the caller's counts; false when a frame holds more rows than the ring has
inline bool columns(int M, int frames, int B, const int (&cnt)[kMaxK], Cols* c) {
  c->M = M;
  c->K = frames;
  c->total = M;
  for (int k = 0; k < kMaxK; ++k) {
    c->cnt[k] = k < frames ? cnt[k] : 0;
    if (c->cnt[k] < 0 || c->cnt[k] > B) return false;
    c->total += c->cnt[k];
  }
  return true;
}

#define QDTRACK_UNSUPPORTED(who) who ": at most 1024 detections, 4096 slots, width 256, 1024 backdrops in each of 4 frames"

}  // namespace qdtrack

extern "C" {

static const char* g_qdtrack_last = "";

const char* qdtrack_hip_last_kernel(void) { return g_qdtrack_last; }

size_t qdtrack_hip_state_offset(int field, int capacity, int D, int backdrop_capacity, int backdrop_frames) {
  if (field < 0 || field > QDTRACK_HIP_STATE_FIELDS || capacity < 1 || D < 1 || backdrop_capacity < 1 || backdrop_frames < 0) return 0;
  return qdtrack::sizes(capacity, D, backdrop_capacity, backdrop_frames).offset(field);
}

int qdtrack_hip_prepare_f32(const float* bboxes, int n, float obj_score_thr, float nms_backdrop_iou_thr, float nms_class_iou_thr,
                            int* order, float* iou, unsigned char* valid, void* stream) {
  using namespace qdtrack;
  if (n < 0) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qdtrack_prepare: bad dimensions");
  if (n > kMaxN) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "qdtrack_prepare: at most 1024 detections");
  if (n == 0) return 0;
  if (!bboxes || !order || !iou || !valid) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "qdtrack_prepare: null pointer argument");
  hipLaunchKernelGGL(rank, dim3((unsigned)msda::ceil_div(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, bboxes, n, order);
  hipLaunchKernelGGL(iou_valid, dim3((unsigned)msda::ceil_div(n, kWaves)), dim3(kThreads), 0, (hipStream_t)stream, bboxes, order, n,
                     obj_score_thr, nms_backdrop_iou_thr, nms_class_iou_thr, iou, valid);
  if (const int e = msda::launch_status()) return e;
  g_qdtrack_last = "qdtrack_prepare";
  return 0;
}

int qdtrack_hip_scores_f32(const float* embeds, const long long* labels, const int* order, const unsigned char* valid, const void* state,
                           int n, int M, int b0, int b1, int b2, int b3, int capacity, int D, int backdrop_capacity,
                           int backdrop_frames, int with_cats, float* row_stats, float* scores, void* stream) {
  using namespace qdtrack;
  if (!geometry_ok(n, M, capacity, D, backdrop_capacity, backdrop_frames))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qdtrack_scores: bad dimensions");
  if (!sizes_ok(n, capacity, D, backdrop_capacity, backdrop_frames)) 
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, QDTRACK_UNSUPPORTED("qdtrack_scores"));
  Cols c;
  if (!columns(M, backdrop_frames, backdrop_capacity, {b0, b1, b2, b3}, &c))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qdtrack_scores: a backdrop frame's rows must lie in [0, backdrop_capacity]");
  if (n == 0 || c.total == 0) return 0;
  if (!embeds || !labels || !order || !valid || !state || !row_stats || !scores)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "qdtrack_scores: null pointer argument");
  const State s = view(state, capacity, D, backdrop_capacity, backdrop_frames);
  const int vec = bank::vec_rows(D, {embeds, s.embed, s.bd_embed});
  hipLaunchKernelGGL(feats_rows, dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, embeds, order, valid, s, c, D,
                     backdrop_capacity, vec, scores, row_stats);
  hipLaunchKernelGGL(cols_final, dim3((unsigned)msda::ceil_div(c.total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, labels, order,
                     valid, row_stats, s, c, n, backdrop_capacity, with_cats ? 1 : 0, scores);
  if (const int e = msda::launch_status()) return e;
  g_qdtrack_last = "qdtrack_scores";
  return 0;
}

int qdtrack_hip_associate_f32(const float* scores, const unsigned char* valid, const int* order, const float* bboxes, const float* iou,
                              const void* state, void* next_state, int n, int M, int b0, int b1, int b2, int b3, int capacity, int D,
                              int backdrop_capacity, int backdrop_frames, float match_score_thr, float obj_score_thr, float nms_conf_thr,
                              float init_score_thr, float nms_backdrop_iou_thr, int frame_id, int memo_tracklet_frames, int* plan,
                              long long* result, void* stream) {
  using namespace qdtrack;
  if (!geometry_ok(n, M, capacity, D, backdrop_capacity, backdrop_frames) || !bank::fits(n, M, capacity) || n > backdrop_capacity)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qdtrack_associate: bad dimensions (M + n must fit the capacity, n the backdrop capacity)");
  if (!sizes_ok(n, capacity, D, backdrop_capacity, backdrop_frames)) 
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, QDTRACK_UNSUPPORTED("qdtrack_associate"));
  Cols c;
  if (!columns(M, backdrop_frames, backdrop_capacity, {b0, b1, b2, b3}, &c))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qdtrack_associate: a backdrop frame's rows must lie in [0, backdrop_capacity]");
  if (!state || !next_state || !plan || !result || state == next_state ||
      (n > 0 && (!valid || !order || !bboxes || !iou || (M > 0 && !scores))))
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "qdtrack_associate: null pointer argument, or the next state is the state");
  const State s = view(state, capacity, D, backdrop_capacity, backdrop_frames);
  const State t = view(next_state, capacity, D, backdrop_capacity, backdrop_frames);
  hipLaunchKernelGGL(associate, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, scores, valid, order, bboxes, iou, s, c, t.meta, n,
                     capacity, backdrop_capacity, match_score_thr, obj_score_thr, nms_conf_thr, init_score_thr, nms_backdrop_iou_thr,
                     frame_id, memo_tracklet_frames, plan, result);
  if (const int e = msda::launch_status()) return e;
  g_qdtrack_last = "qdtrack_associate";
  return 0;
}

int qdtrack_hip_update_f32(const float* embeds, const float* bboxes, const long long* labels, const int* order, const int* plan,
                           const long long* result, const void* state, void* next_state, int n, int M, int b0, int b1, int b2, int b3,
                           int capacity, int D, int backdrop_capacity, int backdrop_frames, float keep_weight, float momentum,
                           int frame_id, void* stream) {
  using namespace qdtrack;
  if (!geometry_ok(n, M, capacity, D, backdrop_capacity, backdrop_frames) || !bank::fits(n, M, capacity) || n > backdrop_capacity)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qdtrack_update: bad dimensions (M + n must fit the capacity, n the backdrop capacity)");
  if (!sizes_ok(n, capacity, D, backdrop_capacity, backdrop_frames)) 
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, QDTRACK_UNSUPPORTED("qdtrack_update"));
  if (state == next_state) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qdtrack_update: the next state must be another buffer");
  Cols c;
  if (!columns(M, backdrop_frames, backdrop_capacity, {b0, b1, b2, b3}, &c))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qdtrack_update: a backdrop frame's rows must lie in [0, backdrop_capacity]");
  if (!state || !next_state || !plan || !result || (n > 0 && (!embeds || !bboxes || !labels || !order)))
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "qdtrack_update: null pointer argument");
  int moving = 0;
  for (int k = 0; k + 1 < backdrop_frames; ++k) moving += c.cnt[k];
  const int blocks = M + n + moving;
  if (blocks > 0) {
    const State a = view(state, capacity, D, backdrop_capacity, backdrop_frames);
    const State b = view(next_state, capacity, D, backdrop_capacity, backdrop_frames);
    hipLaunchKernelGGL(update, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, embeds, bboxes, labels, order, plan, result,
                       a, b, c, n, capacity, D, backdrop_capacity, keep_weight, momentum, frame_id);
    if (const int e = msda::launch_status()) return e;
  }
  g_qdtrack_last = "qdtrack_update";
  return 0;
}

}  // extern "C"
