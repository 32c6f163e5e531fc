// Two-stage query selection: proposal scoring over every row of the encoder memory, and the box head over the rows top-k
// picked -- see include/dynmask_hip.h (qsel_scores_hip_f32, qsel_boxes_hip_f32).
//
// Both kernels share the row-tile routine of row_tile.hpp.  A workgroup (4 waves) owns a tile of 32 rows, 256 features each, in
// LDS:
//
//   load      wave w fetches rows w, w + 4, ... (one 1 KB row per wave-wide float4 load); a padded row, a row whose proposal is
//             invalid, and a row past the end are zeros;
//   linear    Y = X W^T + bias with v_mfma_f32_32x32x2_f32: wave w owns output features [64 w, 64 w + 64) as two 32 x 32
//             accumulator tiles (row of the tile in the registers, feature on the lane).  The weight ([out, in] row-major, as
//             nn.Linear keeps it) is streamed through LDS in chunks of 16 input features; the next chunk travels in registers
//             while the current one is multiplied.  Every row sees the same k order (the MFMA's), so a row's result does not
//             depend on its place in the tile.  Y overwrites X;
//   norm      wave w normalises rows w, w + 4, ... with the two-pass LayerNorm of layernorm.hip.
//
// The scoring kernel then takes the dot product of each normalised row with the image's class vector (one wave per row, a
// butterfly sum), scales, adds the bias, clamps, and optionally writes the normalised row.  The box kernel runs the same routine
// on gathered rows, then two more `linear` steps with ReLU, the 256 -> 4 layer as four butterfly sums per row, adds the
// proposal's logit and writes the boxes and their sigmoid.  Exact fp32, fixed summation orders, no atomics: bitwise repeatable.
#include "../../include/dynmask_hip.h"

#include <math.h>

#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "row_tile.hpp"

namespace qsel {

using namespace row_tile;
using msda::wave_sum;

struct Geometry {
  const unsigned char* __restrict__ mask;    // [B, S], nonzero = padded
  const long long* __restrict__ shapes;      // [n_levels, 2] (H, W)
  const float* __restrict__ valid_wh;        // [B, n_levels, 2] (valid_W, valid_H)
  int n_levels;
  long long S;
};

struct Proposal {
  bool live;            // not padded and valid: the row is read and its logit is finite
  float cx, cy, wh;
};

// The proposal of token s of image b.  cx and cy are IEEE divisions; valid iff cx, cy, w, h all lie strictly in (0.01, 0.99).
__device__ __forceinline__ Proposal proposal_of(const Geometry& g, int b, long long s) {
  Proposal p{false, 0.f, 0.f, 0.f};
  if (s < 0 || s >= g.S) return p;
  long long start = 0;
  for (int l = 0; l < g.n_levels; ++l) {
    const long long H = g.shapes[2 * l], W = g.shapes[2 * l + 1], n = H * W;
    if (s < start + n) {
      const long long r = s - start, y = r / W, x = r - y * W;
      const float vw = g.valid_wh[((long long)b * g.n_levels + l) * 2], vh = g.valid_wh[((long long)b * g.n_levels + l) * 2 + 1];
      p.cx = __fdiv_rn((float)x + 0.5f, vw);
      p.cy = __fdiv_rn((float)y + 0.5f, vh);
      p.wh = ldexpf(0.05f, l);
      const bool valid = p.cx > 0.01f && p.cx < 0.99f && p.cy > 0.01f && p.cy < 0.99f && p.wh > 0.01f && p.wh < 0.99f;
      p.live = valid && g.mask[(long long)b * g.S + s] == 0;
      return p;
    }
    start += n;
  }
  return p;
}

__device__ __forceinline__ float logit_of(float v) { return logf(__fdiv_rn(v, 1.f - v)); }

// LayerNorm of one tile row by one wave (biased variance, eps inside the square root, two passes); the lane's four features.
__device__ __forceinline__ f32x4 norm_row(const float* __restrict__ xrow, const float* __restrict__ gamma,
                                          const float* __restrict__ beta, float eps, int lane) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(xrow + lane * 4);
  const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) / (float)kD;
  float sq = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float dlt = v[e] - mean;
    sq += dlt * dlt;
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)kD + eps);
  const f32x4 g = reinterpret_cast<const f32x4*>(gamma)[lane], b = reinterpret_cast<const f32x4*>(beta)[lane];
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = (v[e] - mean) * rstd * g[e] + b[e];
  return r;
}

// Rows [first, first + 32) of the flattened [B * S] memory: linear, LayerNorm, class score.
__global__ void __launch_bounds__(kThreads)
scores(const float* __restrict__ memory, Geometry g, const float* __restrict__ enc_w, const float* __restrict__ enc_b,
       const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps, const float* __restrict__ class_vec,
       long long class_vec_stride, const float* __restrict__ class_bias, long long class_bias_stride,
       const float* __restrict__ scale, float clamp, long long total, float* __restrict__ logits,
       float* __restrict__ output_memory) {
  __shared__ __attribute__((aligned(16))) float Xs[kRows][kPitch];
  __shared__ __attribute__((aligned(16))) float Ws[kD][kWPitch];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long first = (long long)blockIdx.x * kRows;
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int row = wv + r * (kThreads / 64);
    const long long n = first + row;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n < total) {
      const int b = (int)(n / g.S);
      if (proposal_of(g, b, n - (long long)b * g.S).live) v = *reinterpret_cast<const f32x4*>(memory + n * kD + lane * 4);
    }
    *reinterpret_cast<f32x4*>(&Xs[row][lane * 4]) = v;
  }
  linear_tile<false>(Xs, Ws, enc_w, enc_b, tid);
  const float sc = scale ? scale[0] : 1.f;
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int row = wv + r * (kThreads / 64);
    const long long n = first + row;
    if (n >= total) continue;              // wave-uniform
    const int b = (int)(n / g.S);
    const f32x4 y = norm_row(Xs[row], ln_w, ln_b, eps, lane);
    if (output_memory) *reinterpret_cast<f32x4*>(output_memory + n * kD + lane * 4) = y;
    const f32x4 cv = *reinterpret_cast<const f32x4*>(class_vec + b * class_vec_stride + lane * 4);
    float s = __fdiv_rn(wave_sum(dot4(y, cv)), sc) + class_bias[b * class_bias_stride];
    if (clamp > 0.f) s = fminf(fmaxf(s, -clamp), clamp);
    if (lane == 0) logits[n] = s;
  }
}

// Entries [first, first + 32) of the flattened [B * K] index list: gathered rows through linear, LayerNorm and the box MLP.
__global__ void __launch_bounds__(kThreads)
boxes(const float* __restrict__ memory, Geometry g, const float* __restrict__ enc_w, const float* __restrict__ enc_b,
      const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps, const long long* __restrict__ idx, long long K,
      const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
      const float* __restrict__ w3, const float* __restrict__ b3, long long total, float* __restrict__ coords,
      float* __restrict__ points) {
  __shared__ __attribute__((aligned(16))) float Xs[kRows][kPitch];
  __shared__ __attribute__((aligned(16))) float Ws[kD][kWPitch];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long first = (long long)blockIdx.x * kRows;
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int row = wv + r * (kThreads / 64);
    const long long n = first + row;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (n < total) {
      const int b = (int)(n / K);
      const long long s = idx[n];          // an index outside [0, S) is treated as a padded row
      if (proposal_of(g, b, s).live) v = *reinterpret_cast<const f32x4*>(memory + ((long long)b * g.S + s) * kD + lane * 4);
    }
    *reinterpret_cast<f32x4*>(&Xs[row][lane * 4]) = v;
  }
  linear_tile<false>(Xs, Ws, enc_w, enc_b, tid);
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int row = wv + r * (kThreads / 64);
    const f32x4 y = norm_row(Xs[row], ln_w, ln_b, eps, lane);      // rows past the end too: finite, never stored
    *reinterpret_cast<f32x4*>(&Xs[row][lane * 4]) = y;
  }
  linear_tile<true>(Xs, Ws, w1, b1, tid);
  linear_tile<true>(Xs, Ws, w2, b2, tid);
  f32x4 w3r[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) w3r[c] = *reinterpret_cast<const f32x4*>(w3 + c * kD + lane * 4);
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int row = wv + r * (kThreads / 64);
    const long long n = first + row;
    if (n >= total) continue;              // wave-uniform
    const f32x4 h = *reinterpret_cast<const f32x4*>(&Xs[row][lane * 4]);
    f32x4 out;
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = wave_sum(dot4(h, w3r[c])) + b3[c];
    const Proposal p = proposal_of(g, (int)(n / K), idx[n]);
    const float inf = __builtin_inff();
    out[0] += p.live ? logit_of(p.cx) : inf;
    out[1] += p.live ? logit_of(p.cy) : inf;
    const float lwh = p.live ? logit_of(p.wh) : inf;
    out[2] += lwh;
    out[3] += lwh;
    if (lane == 0) {
      f32x4 sg;
#pragma unroll
      for (int c = 0; c < 4; ++c) sg[c] = 1.f / (1.f + expf(-out[c]));      // +inf -> exactly 1
      *reinterpret_cast<f32x4*>(coords + n * 4) = out;
      *reinterpret_cast<f32x4*>(points + n * 4) = sg;
    }
  }
}

}  // namespace qsel

extern "C" {

static const char* g_qsel_last = "";

const char* qsel_hip_last_kernel(void) { return g_qsel_last; }

static int qsel_check_common(const char* who, int batch, long long S, int n_levels, int d_model) {
  if (batch < 0 || S < 0 || n_levels <= 0 || d_model <= 0) return msda::set_error(DYNMASK_ERR_BAD_DIMS, who);
  if (d_model != qsel::kD) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "qsel: d_model must be 256");
  if (batch > 0 && S > 0 && (S >= (1ll << 31) || (long long)batch * S >= (1ll << 36)))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qsel: problem too large");
  return 0;
}

int qsel_scores_hip_f32(const float* memory, const unsigned char* padding_mask, const long long* spatial_shapes, int n_levels,
                        const float* valid_wh, const float* enc_weight, const float* enc_bias, const float* ln_weight,
                        const float* ln_bias, float eps, const float* class_vec, long long class_vec_stride,
                        const float* class_bias, long long class_bias_stride, const float* scale, float clamp, int batch,
                        long long S, int d_model, float* logits, float* output_memory, void* stream) {
  if (const int rc = qsel_check_common("qsel_scores: bad dimensions", batch, S, n_levels, d_model)) return rc;
  if (class_vec_stride < 0 || class_bias_stride < 0 || class_vec_stride % 4 != 0)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qsel_scores: class strides must be >= 0, the vector's a multiple of 4");
  const long long total = (long long)batch * S;
  if (total == 0) return 0;
  if (!memory || !padding_mask || !spatial_shapes || !valid_wh || !enc_weight || !enc_bias || !ln_weight || !ln_bias ||
      !class_vec || !class_bias || !logits)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "qsel_scores: null pointer argument");
  if (!msda::aligned16({memory, enc_weight, ln_weight, ln_bias, class_vec, output_memory}))
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "qsel_scores: memory, weights, class_vec and output_memory must be 16-byte aligned");
  const qsel::Geometry g{padding_mask, spatial_shapes, valid_wh, n_levels, S};
  const dim3 grid((unsigned)((total + qsel::kRows - 1) / qsel::kRows)), block(qsel::kThreads);
  hipLaunchKernelGGL(qsel::scores, grid, block, 0, (hipStream_t)stream, memory, g, enc_weight, enc_bias, ln_weight, ln_bias, eps,
                     class_vec, class_vec_stride, class_bias, class_bias_stride, scale, clamp, total, logits, output_memory);
  if (const int e = msda::launch_status()) return e;
  g_qsel_last = output_memory ? "qsel_scores<memory>" : "qsel_scores";
  return 0;
}

int qsel_boxes_hip_f32(const float* memory, const unsigned char* padding_mask, const long long* spatial_shapes, int n_levels,
                       const float* valid_wh, const float* enc_weight, const float* enc_bias, const float* ln_weight,
                       const float* ln_bias, float eps, const long long* idx, long long K, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* w3, const float* b3, int batch, long long S, int d_model,
                       float* coords_unact, float* reference_points, void* stream) {
  if (const int rc = qsel_check_common("qsel_boxes: bad dimensions", batch, S, n_levels, d_model)) return rc;
  if (K < 0 || (batch > 0 && K >= (1ll << 36) / batch)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "qsel_boxes: bad K");
  const long long total = (long long)batch * K;
  if (total == 0) return 0;
  if (!memory || !padding_mask || !spatial_shapes || !valid_wh || !enc_weight || !enc_bias || !ln_weight || !ln_bias || !idx ||
      !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !coords_unact || !reference_points)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "qsel_boxes: null pointer argument");
  if (!msda::aligned16({memory, enc_weight, ln_weight, ln_bias, w1, w2, w3, coords_unact, reference_points}))
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "qsel_boxes: memory, weights and outputs must be 16-byte aligned");
  const qsel::Geometry g{padding_mask, spatial_shapes, valid_wh, n_levels, S};
  const dim3 grid((unsigned)((total + qsel::kRows - 1) / qsel::kRows)), block(qsel::kThreads);
  hipLaunchKernelGGL(qsel::boxes, grid, block, 0, (hipStream_t)stream, memory, g, enc_weight, enc_bias, ln_weight, ln_bias, eps, idx,
                     K, w1, b1, w2, b2, w3, b3, total, coords_unact, reference_points);
  if (const int e = msda::launch_status()) return e;
  g_qsel_last = "qsel_boxes";
  return 0;
}

}  // extern "C"
