// The element-wise blocks of a transformer layer under training -- see include/dynmask_hip.h:
//   dropout_add_layernorm  z = residual + keep c x, out = LayerNorm(z) gamma + beta; z is what the backward keeps
//   its backward           mean and rstd recomputed from z (row_stats: the forward's expressions), the mask recomputed
//   relu_dropout           out = keep c max(h, 0); the backward reads out alone
//   row_dropout_keep       the decisions written out, for tests
// Every keep decision is philox::row_words(seed, offset, row, column / 4): one call per lane's float4, no mask is stored.
//
// All memory bound.  The LayerNorm kernels hold a row per wave in registers as layernorm.hip does (float4 chunks of 64 lanes,
// coalesced 16-byte accesses).  The backward gives a workgroup kBwdRows consecutive rows -- a function of `rows` alone, never of
// the device -- and a lane sums its columns of grad_gamma and grad_beta over them in float64; the four waves add up through
// LDS in wave order and the workgroup writes one row of float64 partials, which reduce_partials adds in index order
// (16 contiguous segments, then the segments in order).  No atomics: the bits do not depend on the machine or the run.
#include "../../include/dynmask_hip.h"
#include "../../include/layernorm_hip.h"   // the LAYERNORM_ERR_* codes

#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "philox.hpp"

namespace layer_train {

using msda::f32x4;
using wave_ops::wave_sum;

constexpr int kThreads = 256, kWaves = kThreads / 64, kMaxChunks = 16;   // 16 float4 per lane = 4096 features
constexpr int kBwdRows = 32;                       // rows of one backward workgroup = rows of one row of partials
constexpr int kMaxFlatFeatures = 65536;            // relu_dropout and the export
constexpr int kSegments = 16, kColumns = 16;       // reduce_partials: a workgroup adds 16 columns in 16 segments

// c x where kept, 0 where dropped
__device__ __forceinline__ f32x4 dropped(const f32x4& x, const philox::Words& w, uint32_t threshold, float scale) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = w.w[e] >= threshold ? x[e] * scale : 0.f;
  return r;
}

// The forward below is layernorm.hip's add_layernorm line by line, with the dropout and the store of z added: at p == 0 its `out` has
// to be that kernel's bit for bit, which holds only while the compiler contracts the same products and sums in both, so the text
// is kept the same rather than shared through a function (tests/test_layer_train_gpu.py compares the bits at every chunk count).
template <int CHUNKS, bool DROP>   // float4 chunks per lane: features <= CHUNKS * 256
__global__ void __launch_bounds__(kThreads)
dropout_add_layernorm_train(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ gamma,
                            const float* __restrict__ beta, float eps, long long rows, int features, philox::Dropout drop,
                            float* __restrict__ z, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nvec = features / 4;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + row * features);
  const f32x4* rr = res ? reinterpret_cast<const f32x4*>(res + row * features) : nullptr;
  f32x4* zr = reinterpret_cast<f32x4*>(z + row * features);
  [[maybe_unused]] philox::Stream ps{};
  if constexpr (DROP) ps = philox::stream_of(drop);
  f32x4 v[CHUNKS];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int i = c * 64 + lane;
    v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < nvec) {
      v[c] = xr[i];
      if constexpr (DROP) v[c] = dropped(v[c], philox::row_words(ps, (uint32_t)row, (uint32_t)i), drop.threshold, drop.scale);
      if (rr) v[c] += rr[i];
      zr[i] = v[c];
      sum += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
    }
  }
  const float mean = wave_sum(sum) / (float)features;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int i = c * 64 + lane;
    if (i < nvec) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dlt = v[c][e] - mean;
        sq += dlt * dlt;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)features + eps);
  f32x4* orow = reinterpret_cast<f32x4*>(out + row * features);
  const f32x4* gv = reinterpret_cast<const f32x4*>(gamma);
  const f32x4* bv = reinterpret_cast<const f32x4*>(beta);
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int i = c * 64 + lane;
    if (i < nvec) {
      f32x4 r;
      const f32x4 g = gamma ? gv[i] : f32x4{1.f, 1.f, 1.f, 1.f};
      const f32x4 b = beta ? bv[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = (v[c][e] - mean) * rstd * g[e] + b[e];
      orow[i] = r;
    }
  }
}

// mean and rstd of a row held as v[c] = float4 number c * 64 + lane (zero past nvec): the forward's expressions in its order
template <int CHUNKS>
__device__ __forceinline__ void row_stats(const f32x4 (&v)[CHUNKS], int lane, int nvec, int features, float eps, float& mean,
                                          float& rstd) {
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    if (c * 64 + lane < nvec) sum += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
  }
  mean = wave_sum(sum) / (float)features;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    if (c * 64 + lane < nvec) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dlt = v[c][e] - mean;
        sq += dlt * dlt;
      }
    }
  }
  rstd = rsqrtf(wave_sum(sq) / (float)features + eps);
}

// g = grad_out gamma, xh = (z - mean) rstd:  grad_z = rstd (g - mean g - xh mean (g xh)).  PARAMS: the workgroup's column sums
// of grad_out xh and grad_out as float64, row blockIdx.x of `partials` ([blocks][2][features]).
template <int CHUNKS, bool DROP, bool PARAMS>
__global__ void __launch_bounds__(kThreads)
dropout_add_layernorm_bwd(const float* __restrict__ grad_out, const float* __restrict__ z, const float* __restrict__ gamma, float eps,
                          long long rows, int features, philox::Dropout drop, float* __restrict__ grad_x,
                          float* __restrict__ grad_res, double* __restrict__ partials) {
  extern __shared__ double red[];   // PARAMS: [2][features]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nvec = features / 4;
  const long long row0 = (long long)blockIdx.x * kBwdRows;
  [[maybe_unused]] philox::Stream ps{};
  if constexpr (DROP) ps = philox::stream_of(drop);
  [[maybe_unused]] double acc_g[PARAMS ? CHUNKS : 1][4], acc_b[PARAMS ? CHUNKS : 1][4];
  if constexpr (PARAMS) {
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc_g[c][e] = acc_b[c][e] = 0.0;
    }
  }
  for (int k = wv; k < kBwdRows; k += kWaves) {
    const long long row = row0 + k;
    if (row >= rows) break;   // the whole wave; the barriers are below the loop
    const f32x4* zr = reinterpret_cast<const f32x4*>(z + row * features);
    const f32x4* gr = reinterpret_cast<const f32x4*>(grad_out + row * features);
    f32x4 v[CHUNKS], g[CHUNKS];
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = c * 64 + lane;
      v[c] = g[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < nvec) {
        v[c] = zr[i];
        g[c] = gr[i];
      }
    }
    float mean, rstd;
    row_stats<CHUNKS>(v, lane, nvec, features, eps, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = c * 64 + lane;
      if (i < nvec) {
        const f32x4 gm = gamma ? reinterpret_cast<const f32x4*>(gamma)[i] : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = (v[c][e] - mean) * rstd;
          if constexpr (PARAMS) {
            acc_g[c][e] += (double)g[c][e] * (double)xh;
            acc_b[c][e] += (double)g[c][e];
          }
          const float gw = g[c][e] * gm[e];
          s1 += gw;
          s2 += gw * xh;
          v[c][e] = xh;
          g[c][e] = gw;
        }
      }
    }
    const float m1 = wave_sum(s1) / (float)features, m2 = wave_sum(s2) / (float)features;
    f32x4* dxr = grad_x ? reinterpret_cast<f32x4*>(grad_x + row * features) : nullptr;
    f32x4* drr = grad_res ? reinterpret_cast<f32x4*>(grad_res + row * features) : nullptr;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      const int i = c * 64 + lane;
      if (i < nvec) {
        f32x4 dz;
#pragma unroll
        for (int e = 0; e < 4; ++e) dz[e] = rstd * (g[c][e] - m1 - v[c][e] * m2);
        if (drr) drr[i] = dz;
        if (dxr) {
          if constexpr (DROP) dz = dropped(dz, philox::row_words(ps, (uint32_t)row, (uint32_t)i), drop.threshold, drop.scale);
          dxr[i] = dz;
        }
      }
    }
  }
  if constexpr (PARAMS) {
    for (int w = 0; w < kWaves; ++w) {   // wave 0 stores, waves 1 .. 3 add in order
      if (wv == w) {
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
          const int i = c * 64 + lane;
          if (i < nvec) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              double* pg = red + 4 * i + e;
              double* pb = red + features + 4 * i + e;
              *pg = w == 0 ? acc_g[c][e] : *pg + acc_g[c][e];
              *pb = w == 0 ? acc_b[c][e] : *pb + acc_b[c][e];
            }
          }
        }
      }
      __syncthreads();
    }
    double* dst = partials + (long long)blockIdx.x * 2 * features;
    for (int i = threadIdx.x; i < 2 * features; i += kThreads) dst[i] = red[i];
  }
}

// grad_gamma (blockIdx.y == 0) or grad_beta (1) of 16 columns: 16 contiguous segments of the rows of partials, each added in
// index order, then the segments in order.
__global__ void __launch_bounds__(kThreads)
reduce_partials(const double* __restrict__ partials, int blocks, int features, float* __restrict__ grad_gamma,
                float* __restrict__ grad_beta) {
  __shared__ double seg[kSegments][kColumns];
  const int cl = threadIdx.x % kColumns, s = threadIdx.x / kColumns;
  const int col = blockIdx.x * kColumns + cl, which = blockIdx.y;
  float* dst = which ? grad_beta : grad_gamma;
  const bool live = dst && col < features;
  const int per = (blocks + kSegments - 1) / kSegments;
  const int b0 = s * per, b1 = min(blocks, b0 + per);
  double a = 0.0;
  if (live)
    for (int b = b0; b < b1; ++b) a += partials[((long long)b * 2 + which) * features + col];
  seg[s][cl] = a;
  __syncthreads();
  if (live && s == 0) {
    double t = seg[0][cl];
    for (int k = 1; k < kSegments; ++k) t += seg[k][cl];
    dst[col] = (float)t;
  }
}

// (row, column / 4) of float4 number idx of a contiguous [rows, 4 nvec] tensor
__device__ __forceinline__ void row_col4(long long idx, int nvec, bool narrow, uint32_t& row, uint32_t& col4) {
  if (narrow) {   // idx < 2^32: the 32-bit division
    row = (uint32_t)idx / (uint32_t)nvec;
    col4 = (uint32_t)idx - row * (uint32_t)nvec;
  } else {
    const long long r = idx / nvec;
    row = (uint32_t)r;
    col4 = (uint32_t)(idx - r * nvec);
  }
}

template <bool DROP>
__global__ void __launch_bounds__(kThreads)
relu_dropout(const f32x4* __restrict__ h, long long total, int nvec, philox::Dropout drop, f32x4* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  f32x4 v = h[idx];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  if constexpr (DROP) {
    uint32_t row, col4;
    row_col4(idx, nvec, total < (1ll << 32), row, col4);
    v = dropped(v, philox::row_words(philox::stream_of(drop), row, col4), drop.threshold, drop.scale);
  }
  out[idx] = v;
}

__global__ void __launch_bounds__(kThreads)
relu_dropout_bwd(const f32x4* __restrict__ grad_out, const f32x4* __restrict__ out, long long total, float scale,
                 f32x4* __restrict__ grad_h) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const f32x4 g = grad_out[idx], o = out[idx];
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = o[e] > 0.f ? g[e] * scale : 0.f;
  grad_h[idx] = r;
}

__global__ void __launch_bounds__(kThreads)
row_dropout_keep(philox::Dropout drop, long long total, int nvec, uint32_t* __restrict__ keep) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  uint32_t row, col4;
  row_col4(idx, nvec, total < (1ll << 32), row, col4);
  const philox::Words w = philox::row_words(philox::stream_of(drop), row, col4);
  uint32_t bytes = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) bytes |= (uint32_t)(w.w[t] >= drop.threshold) << (8 * t);
  keep[idx] = bytes;   // bytes (row, 4 col4 .. 4 col4 + 3): features % 4 == 0, so float4 idx is uint32 idx
}

// ---- host side -----------------------------------------------------------------------------------
// The checks the entry points share: 0 and `drop` filled, or the refusal's code.
inline int geometry(const char* who, long long rows, int features, int max_features, float p, const unsigned long long* seed,
                    bool takes_seed, philox::Dropout& drop) {
  static thread_local char text[160];
  const auto refuse = [&](int code, const char* what) {
    snprintf(text, sizeof text, "%s: %s", who, what);
    return msda::set_error(code, text);
  };
  if (rows < 0 || features <= 0) return refuse(LAYERNORM_ERR_BAD_DIMS, "bad dimensions");
  if (rows >= (1ll << 32)) return refuse(LAYERNORM_ERR_BAD_DIMS, "rows must be below 2^32");
  if (features % 4 != 0 || features > max_features)
    return refuse(LAYERNORM_ERR_UNSUPPORTED, max_features == kMaxChunks * 256 ? "features must be a multiple of 4 and <= 4096"
                                                                              : "features must be a multiple of 4 and <= 65536");
  if (!(p >= 0.f && p < 1.f)) return refuse(LAYERNORM_ERR_BAD_DIMS, "p must be in [0, 1)");
  if (takes_seed && p > 0.f && !seed) return refuse(LAYERNORM_ERR_NULL_POINTER, "p > 0 needs the seed");
  drop.seed = seed;
  drop.threshold = (uint32_t)llrint((double)p * 4294967296.0);
  drop.scale = 1.0f / (1.0f - p);
  return 0;
}

inline int null_pointer(const char* what) { return msda::set_error(LAYERNORM_ERR_NULL_POINTER, what); }

// grid of a flat kernel over `total` float4, or 0 when it does not fit
inline long long flat_blocks(long long total) {
  const long long blocks = msda::ceil_div(total, (long long)kThreads);
  return blocks < (1ll << 31) ? blocks : 0;
}

inline long long bwd_blocks(long long rows) { return msda::ceil_div(rows, (long long)kBwdRows); }

}  // namespace layer_train

extern "C" {

int dropout_add_layernorm_hip_train_f32(const float* x, const float* residual, const float* gamma, const float* beta, float eps,
                                        long long rows, int features, float p, const unsigned long long* seed, float* z, float* out,
                                        void* stream) {
  using namespace layer_train;
  philox::Dropout drop;
  const int rc = geometry("dropout_add_layernorm_train", rows, features, kMaxChunks * 256, p, seed, true, drop);
  if (rc) return rc;
  if (rows == 0) return 0;
  if (!x || !z || !out) return null_pointer("dropout_add_layernorm_train: null pointer argument");
  const dim3 grid((unsigned)msda::ceil_div(rows, (long long)kWaves)), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (features / 4 + 63) / 64;
#define LT_LAUNCH(C, D) \
  hipLaunchKernelGGL((dropout_add_layernorm_train<C, D>), grid, block, 0, st, x, residual, gamma, beta, eps, rows, features, drop, z, out)
#define LT_CHUNKS(D)                  \
  if (chunks <= 1) LT_LAUNCH(1, D);      \
  else if (chunks <= 2) LT_LAUNCH(2, D); \
  else if (chunks <= 4) LT_LAUNCH(4, D); \
  else if (chunks <= 8) LT_LAUNCH(8, D); \
  else LT_LAUNCH(16, D)
  if (p > 0.f) { LT_CHUNKS(true); } else { LT_CHUNKS(false); }
#undef LT_LAUNCH
  return msda::launch_status();
}

size_t dropout_add_layernorm_hip_backward_workspace_bytes(long long rows, int features) {
  if (rows <= 0 || features <= 0 || rows >= (1ll << 32)) return 0;
  return (size_t)layer_train::bwd_blocks(rows) * 2 * (size_t)features * sizeof(double);
}

int dropout_add_layernorm_hip_backward_f32(const float* grad_out, const float* z, const float* gamma, float eps, long long rows,
                                           int features, float p, const unsigned long long* seed, float* grad_x,
                                           float* grad_residual, float* grad_gamma, float* grad_beta, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  using namespace layer_train;
  philox::Dropout drop;
  const int rc = geometry("dropout_add_layernorm_backward", rows, features, kMaxChunks * 256, p, seed, true, drop);
  if (rc) return rc;
  if (rows == 0) return 0;
  if (!grad_out || !z) return null_pointer("dropout_add_layernorm_backward: null pointer argument");
  const bool params = grad_gamma || grad_beta;
  if (params) {
    if (!workspace) return null_pointer("dropout_add_layernorm_backward: null workspace");
    if (workspace_bytes < dropout_add_layernorm_hip_backward_workspace_bytes(rows, features))
      return msda::set_error(LAYERNORM_ERR_WORKSPACE, "dropout_add_layernorm_backward: workspace below its workspace_bytes query");
  }
  if (!params && !grad_x && !grad_residual) return 0;
  const long long blocks = bwd_blocks(rows);
  const dim3 grid((unsigned)blocks), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  double* partials = (double*)workspace;
  const size_t lds = params ? 2 * (size_t)features * sizeof(double) : 0;
  const bool drops = p > 0.f && grad_x;   // the mask enters grad_x alone
  const int chunks = (features / 4 + 63) / 64;
#define LT_LAUNCH(C, D, P)                                                                                                     \
  hipLaunchKernelGGL((dropout_add_layernorm_bwd<C, D, P>), grid, block, lds, st, grad_out, z, gamma, eps, rows, features, drop, \
                     grad_x, grad_residual, partials)
#define LT_SWITCH(C)                               \
  do {                                             \
    if (drops && params) LT_LAUNCH(C, true, true); \
    else if (drops) LT_LAUNCH(C, true, false);     \
    else if (params) LT_LAUNCH(C, false, true);    \
    else LT_LAUNCH(C, false, false);               \
  } while (0)
  if (chunks <= 1) LT_SWITCH(1);
  else if (chunks <= 2) LT_SWITCH(2);
  else if (chunks <= 4) LT_SWITCH(4);
  else if (chunks <= 8) LT_SWITCH(8);
  else LT_SWITCH(16);
#undef LT_SWITCH
#undef LT_LAUNCH
  if (params) {
    const dim3 rgrid((unsigned)msda::ceil_div(features, kColumns), 2);
    hipLaunchKernelGGL(reduce_partials, rgrid, block, 0, st, partials, (int)blocks, features, grad_gamma, grad_beta);
  }
  return msda::launch_status();
}

int relu_dropout_hip_f32(const float* h, long long rows, int features, float p, const unsigned long long* seed, float* out,
                         void* stream) {
  using namespace layer_train;
  philox::Dropout drop;
  const int rc = geometry("relu_dropout", rows, features, kMaxFlatFeatures, p, seed, true, drop);
  if (rc) return rc;
  if (rows == 0) return 0;
  if (!h || !out) return null_pointer("relu_dropout: null pointer argument");
  const long long total = rows * (features / 4), blocks = flat_blocks(total);
  if (!blocks) return msda::set_error(LAYERNORM_ERR_BAD_DIMS, "relu_dropout: too many elements");
  const dim3 grid((unsigned)blocks), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (p > 0.f)
    hipLaunchKernelGGL(relu_dropout<true>, grid, block, 0, st, (const f32x4*)h, total, features / 4, drop, (f32x4*)out);
  else
    hipLaunchKernelGGL(relu_dropout<false>, grid, block, 0, st, (const f32x4*)h, total, features / 4, drop, (f32x4*)out);
  return msda::launch_status();
}

int relu_dropout_hip_backward_f32(const float* grad_out, const float* out, long long rows, int features, float p, float* grad_h,
                                  void* stream) {
  using namespace layer_train;
  philox::Dropout drop;
  const int rc = geometry("relu_dropout_backward", rows, features, kMaxFlatFeatures, p, nullptr, false, drop);
  if (rc) return rc;
  if (rows == 0) return 0;
  if (!grad_out || !out || !grad_h) return null_pointer("relu_dropout_backward: null pointer argument");
  const long long total = rows * (features / 4), blocks = flat_blocks(total);
  if (!blocks) return msda::set_error(LAYERNORM_ERR_BAD_DIMS, "relu_dropout_backward: too many elements");
  hipLaunchKernelGGL(relu_dropout_bwd, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, (const f32x4*)grad_out,
                     (const f32x4*)out, total, drop.scale, (f32x4*)grad_h);
  return msda::launch_status();
}

int row_dropout_hip_keep_u8(const unsigned long long* seed, float p, long long rows, int features, unsigned char* keep,
                            void* stream) {
  using namespace layer_train;
  philox::Dropout drop;
  if (!seed) return null_pointer("row_dropout_keep: null seed");
  const int rc = geometry("row_dropout_keep", rows, features, kMaxFlatFeatures, p, seed, true, drop);
  if (rc) return rc;
  if (rows == 0) return 0;
  if (!keep) return null_pointer("row_dropout_keep: null pointer argument");
  const long long total = rows * (features / 4), blocks = flat_blocks(total);
  if (!blocks) return msda::set_error(LAYERNORM_ERR_BAD_DIMS, "row_dropout_keep: too many elements");
  hipLaunchKernelGGL(row_dropout_keep, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, drop, total, features / 4,
                     (uint32_t*)keep);
  return msda::launch_status();
}

}  // extern "C"
