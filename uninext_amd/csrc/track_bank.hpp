// What the two trackers' memory banks share: tracker.hip (IDOL, models/tracker.py:98-298) and qdtrack.hip (QuasiDense,
// :304-503).  The layout of a bank, the bi-softmax scores of a frame against the memory's columns, the update of the fields
// both banks have, and the launchers' common checks.  Internal, not part of the C ABI.
//
// The scores decide integer outputs and are compared bit for bit, so the INCLUDING FILE MUST HAVE CONTRACTION OFF
// (`#pragma clang fp contract(off)` above the include).  No atomics; every reduction in a fixed order: bitwise repeatable.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

#include <initializer_list>

#include "../../include/dynmask_hip.h"
#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "wave_ops.hpp"

namespace bank {

using wave_ops::wave_max, wave_ops::wave_sum;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxN = MASKPOST_HIP_MAX_MASKS;
constexpr int kMaxC = TRACK_HIP_MAX_CAPACITY;
constexpr int kMaxD = TRACK_HIP_MAX_DIM;
constexpr int kBox = 5;

// ------------------------------------------------------------------------------------------------------------------- layout
// A bank is one buffer of fields, each padded to 16 bytes.  A tracker keeps its table of the fields' sizes and its State.
// the fields both banks have, one entry per slot but for `meta` (the counters; a tracker may append its own)
struct Slots {
  long long* meta;      // count, num_tracklets, ...
  long long* id;        // [C]
  long long* label;     // [C]
  float* bbox;          // [C, 5]
  float* velocity;      // [C, 5]
  int* last_frame;      // [C]
  int* acc_frame;       // [C]
  float* embed;         // [C, D]
};

inline size_t pad16(size_t v) { return (v + 15) / 16 * 16; }

// byte offset of field `field` of a bank with `fields` fields of sizes[]; field == fields: the bank's size
inline size_t offset(const size_t* sizes, int fields, int field) {
  size_t at = 0;
  for (int k = 0; k < field && k < fields; ++k) at += pad16(sizes[k]);
  return at;
}

template <typename T>
inline T* at(const void* base, size_t byte_offset) { return reinterpret_cast<T*>(const_cast<char*>(static_cast<const char*>(base)) + byte_offset); }

// the common fields of a bank at `base`: fields 0 .. 6 in the order of Slots, `embed` at field embed_field
inline void view_slots(Slots* s, const void* base, const size_t* sizes, int fields, int embed_field) {
  s->meta = at<long long>(base, offset(sizes, fields, 0));
  s->id = at<long long>(base, offset(sizes, fields, 1));
  s->label = at<long long>(base, offset(sizes, fields, 2));
  s->bbox = at<float>(base, offset(sizes, fields, 3));
  s->velocity = at<float>(base, offset(sizes, fields, 4));
  s->last_frame = at<int>(base, offset(sizes, fields, 5));
  s->acc_frame = at<int>(base, offset(sizes, fields, 6));
  s->embed = at<float>(base, offset(sizes, fields, embed_field));
}

// ------------------------------------------------------------------------------------------------------------------- scores
// Row i of the bi-softmax by its whole workgroup of kThreads: the dot products of embedding e [D] with the M columns col(m)
// [D] -- a wave forms one at a time, 16-byte loads when `vec` (D a multiple of 4, every row 16-byte aligned) -- stay in an LDS
// row of kRow floats for the row's maximum and its sum of exponentials.  Writes feats[i, :M] and rstat[2 i .. 2 i + 1].
// Every thread of the workgroup calls it.
template <int kRow, typename Col>
__device__ __forceinline__ void score_row(const float* __restrict__ e, Col col, int i, int M, int D, int vec, float* __restrict__ feats,
                                          float* __restrict__ rstat) {
  __shared__ float row[kRow];
  __shared__ float red[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (vec) {
    const int quads = D >> 2;
    msda::f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (lane < quads) a = reinterpret_cast<const msda::f32x4*>(e)[lane];
    for (int m = wv; m < M; m += kWaves) {
      const float* __restrict__ c = col(m);
      float p = 0.f;
      if (lane < quads) {
        const msda::f32x4 b = reinterpret_cast<const msda::f32x4*>(c)[lane];
        p = a[0] * b[0];
        p += a[1] * b[1];
        p += a[2] * b[2];
        p += a[3] * b[3];
      }
      p = wave_sum(p);
      if (lane == 0) row[m] = p;
    }
  } else {
    for (int m = wv; m < M; m += kWaves) {
      const float* __restrict__ c = col(m);
      float p = 0.f;
      for (int d = lane; d < D; d += 64) p += e[d] * c[d];
      p = wave_sum(p);
      if (lane == 0) row[m] = p;
    }
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int m = tid; m < M; m += kThreads) mx = fmaxf(mx, row[m]);
  mx = wave_max(mx);
  if (lane == 0) red[wv] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int m = tid; m < M; m += kThreads) {
    const float f = row[m];
    feats[(size_t)i * M + m] = f;
    sum += expf(f - mx);
  }
  sum = wave_sum(sum);
  if (lane == 0) red[wv] = sum;
  __syncthreads();
  if (tid == 0) {
    rstat[2 * i] = mx;
    rstat[2 * i + 1] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

struct NoGate { __device__ int operator()() const { return 0; } };

// Column m of the bi-softmax by one lane: the column's maximum and sum over the kept rows of scores [n, M] (the feats of
// score_row), then in place v = (row softmax + column softmax) / 2, or gate(i, v) when there is a gate.  make_gate() gives the
// column's gate; it is called between the two passes, where qdtrack.hip has always looked the column's label up.
template <typename MakeGate = NoGate>
__device__ __forceinline__ void col_softmax(const unsigned char* __restrict__ keep, const float* __restrict__ rstat, int n, int M, int m,
                                            float* __restrict__ scores, MakeGate make_gate = MakeGate()) {
  float mx = -INFINITY;
  for (int i = 0; i < n; ++i)
    if (keep[i]) mx = fmaxf(mx, scores[(size_t)i * M + m]);
  float sum = 0.f;
  for (int i = 0; i < n; ++i)
    if (keep[i]) sum += expf(scores[(size_t)i * M + m] - mx);
  [[maybe_unused]] const auto gate = make_gate();
  for (int i = 0; i < n; ++i) {
    if (!keep[i]) continue;
    const float f = scores[(size_t)i * M + m];
    const float d2t = __fdiv_rn(expf(f - rstat[2 * i]), rstat[2 * i + 1]);
    const float t2d = __fdiv_rn(expf(f - mx), sum);
    float v = (d2t + t2d) * 0.5f;
    if constexpr (!__is_same(MakeGate, NoGate)) v = gate(i, v);
    scores[(size_t)i * M + m] = v;
  }
}

// ------------------------------------------------------------------------------------------------------------------- update
// The common fields of slot dst of the NEXT bank b, by a whole workgroup (every thread calls).  `id` and `label` are read by
// thread 0 alone.  kCopy: the detection's embedding goes to copy [D] as well (IDOL's ring).

// a new tracklet from a detection's embedding e [D] and box [5]
template <bool kCopy>
__device__ __forceinline__ void slot_new(const Slots& b, int dst, int D, const float* e, float* copy,
                                         const float* box, const long long& id, const long long& label, int frame_id) {
  const int tid = threadIdx.x;
  for (int d = tid; d < D; d += kThreads) {
    b.embed[(size_t)dst * D + d] = e[d];
    if constexpr (kCopy) copy[d] = e[d];
  }
  if (tid < kBox) {
    b.bbox[dst * kBox + tid] = box[tid];
    b.velocity[dst * kBox + tid] = 0.f;
  }
  if (tid == 0) {
    b.id[dst] = id;
    b.label[dst] = label;
    b.last_frame[dst] = frame_id;
    b.acc_frame[dst] = 0;
  }
}

// slot m of bank a was not seen in this frame: it moves as it is
__device__ __forceinline__ void slot_move(const Slots& a, const Slots& b, int dst, int m, int D) {
  const int tid = threadIdx.x;
  for (int d = tid; d < D; d += kThreads) b.embed[(size_t)dst * D + d] = a.embed[(size_t)m * D + d];
  if (tid < kBox) {
    b.bbox[dst * kBox + tid] = a.bbox[m * kBox + tid];
    b.velocity[dst * kBox + tid] = a.velocity[m * kBox + tid];
  }
  if (tid == 0) {
    b.id[dst] = a.id[m];
    b.label[dst] = a.label[m];
    b.last_frame[dst] = a.last_frame[m];
    b.acc_frame[dst] = a.acc_frame[m];
  }
}

// slot m of bank a matched a detection (tracker.py:111-129, :351-364): the embedding's moving average, the running mean of the
// velocity, one IEEE operation per operation of the reference
template <bool kCopy>
__device__ __forceinline__ void slot_match(const Slots& a, const Slots& b, int dst, int m, int D, const float* e,
                                           float* copy, const float* box, const long long& label,
                                           float keep_weight, float momentum, int frame_id) {
  const int tid = threadIdx.x;
  for (int d = tid; d < D; d += kThreads) {
    b.embed[(size_t)dst * D + d] = keep_weight * a.embed[(size_t)m * D + d] + momentum * e[d];
    if constexpr (kCopy) copy[d] = e[d];
  }
  if (tid < kBox) {
    const float nb = box[tid];
    const int acc = a.acc_frame[m];
    const float v = __fdiv_rn(nb - a.bbox[m * kBox + tid], (float)(frame_id - a.last_frame[m]));
    b.bbox[dst * kBox + tid] = nb;
    b.velocity[dst * kBox + tid] = __fdiv_rn(a.velocity[m * kBox + tid] * (float)acc + v, (float)(acc + 1));
  }
  if (tid == 0) {
    b.id[dst] = a.id[m];
    b.label[dst] = label;
    b.last_frame[dst] = frame_id;
    b.acc_frame[dst] = a.acc_frame[m] + 1;
  }
}

// --------------------------------------------------------------------------------------------------------------------- host
inline bool geometry_ok(int n, int M, int capacity, int D) { return n >= 0 && M >= 0 && capacity >= 1 && D >= 1 && M <= capacity; }
inline bool sizes_ok(int n, int capacity, int D) { return n <= kMaxN && capacity <= kMaxC && D <= kMaxD; }

inline bool fits(int n, int M, int capacity) { return (long long)M + n <= capacity; }      // a new tracklet for any detection
// 1 when score_row may use its 16-byte loads on rows of D floats that start at these pointers
inline int vec_rows(int D, std::initializer_list<const void*> ptrs) { return D % 4 == 0 && msda::aligned16(ptrs) ? 1 : 0; }

}  // namespace bank
