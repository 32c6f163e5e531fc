// The training criterion's two streaming losses -- see include/dynmask_hip.h (criterion_hip_*).
//
//   token focal   one wave per (image, query) row of T <= 256 token logits, four rows per workgroup.  The row's target is a row of
//                 the concatenated positive maps (or zeros), the text mask is read as it is stored: no one-hot tensor, no repeated
//                 mask, no compacted copies.  Forward: every lane adds its terms in float64, the workgroup writes ONE partial sum.
//                 Backward: the same indexing, the gradient recomputed from the logits, exactly 0.0 at masked tokens.
//   mask losses   grid = instances x pixel slices.  A pixel's target is one byte of the padded full-resolution masks at
//                 (start + stride y, start + stride x): no fp32 copy of them, no gathered target tensor.  Forward: four sums per
//                 (instance, slice): focal, sigma(x) t, sigma(x), t.  Backward: both gradients in one pass from the [n, 4] sums.
//   finish        ONE workgroup adds the partial sums in a fixed order (float64) and writes the fp32 results.
//
// No atomics and no "last block finishes" ticket: a sum is the same bits on every call.  The partial sums live in a workspace
// the caller lends (criterion_hip_workspace_bytes).
#include "../../include/dynmask_hip.h"

#include <math.h>
#include <stdint.h>

#include "launch_glue.hpp"
#include "msda_common.hpp"

namespace criterion {

using msda::f32x4;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxT = CRITERION_HIP_MAX_TOKENS;
constexpr int kTargetBlocks = 2048;      // 256 CUs x 8 resident workgroups: what the slices of the mask kernels aim at
constexpr int kMinSlice = 4 * kThreads;  // a slice is at least one 16-byte load per thread

// sigmoid(x), sigmoid(-x) and BCE-with-logits' softplus term log(1 + exp(-|x|)), none of them cancelling at large |x|
struct Sig {
  float p, q, sp;
};
__device__ __forceinline__ Sig sig(float x) {
  const float e = expf(-fabsf(x)), r = 1.f / (1.f + e);
  Sig s;
  s.p = x >= 0.f ? r : e * r;
  s.q = x >= 0.f ? e * r : r;
  s.sp = log1pf(e);
  return s;
}

// alpha_t * ce * (1 - p_t)^2 for a target t in [0, 1]  (gamma == 2)
__device__ __forceinline__ float focal(float x, float t, float alpha, const Sig& s) {
  const float ce = fmaxf(x, 0.f) - x * t + s.sp;
  const float m = s.p * (1.f - t) + s.q * t;                       // 1 - p_t
  return (alpha * t + (1.f - alpha) * (1.f - t)) * (ce * (m * m));
}

// d focal / dx:  alpha_t ((p - t) m^2 + 2 ce m (1 - 2 t) p (1 - p)).  p - t is formed as p (1 - t) - q t: at t = 1 and a
// saturated logit the difference of p and 1 has lost its digits (1e-3 of the gradient at x = 10), -q has not.
__device__ __forceinline__ float focal_grad(float x, float t, float alpha, const Sig& s) {
  const float ce = fmaxf(x, 0.f) - x * t + s.sp;
  const float m = s.p * (1.f - t) + s.q * t;
  const float dm = (1.f - 2.f * t) * (s.p * s.q);
  const float pt = s.p * (1.f - t) - s.q * t;
  return (alpha * t + (1.f - alpha) * (1.f - t)) * (pt * (m * m) + 2.f * (ce * (m * dm)));
}

__device__ __forceinline__ bool counted(const void* mask, int kind, long long at) {
  if (kind == CRITERION_MASK_INT64) return static_cast<const long long*>(mask)[at] > 0;
  if (kind == CRITERION_MASK_BOOL) return static_cast<const unsigned char*>(mask)[at] != 0;
  return true;
}

// ---- token focal loss ----------------------------------------------------------------------------------------------------------
// VEC: T % 4 == 0 and 16-byte aligned bases: lane l takes tokens 4 l .. 4 l + 3.  BWD writes grad instead of summing.
template <bool VEC, bool BWD>
__global__ void __launch_bounds__(kThreads)
token_focal(const float* __restrict__ logits, const void* __restrict__ mask, int mask_kind, const int* __restrict__ row_target,
            const float* __restrict__ pmap, int G, float alpha, int rows, int Q, int T, const float* __restrict__ scale_ptr,
            double* __restrict__ part, float* __restrict__ grad) {
  __shared__ double red[kWaves][1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = blockIdx.x * kWaves + wv;
  double acc[1] = {0.0};
  if (row < rows) {                            // wave-uniform
    const long long base = (long long)row * T;
    const long long mbase = (long long)(row / Q) * T;
    const int tr = row_target[row];
    const float* __restrict__ tgt = (unsigned)tr < (unsigned)G ? pmap + (long long)tr * T : nullptr;
    const float scale = BWD ? *scale_ptr : 0.f;
    if (VEC) {
      const int t0 = 4 * lane;
      if (t0 < T) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(logits + base + t0);
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (tgt) t = *reinterpret_cast<const f32x4*>(tgt + t0);
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!counted(mask, mask_kind, mbase + t0 + e)) continue;
          const Sig s = sig(x[e]);
          if (BWD) g[e] = scale * focal_grad(x[e], t[e], alpha, s);
          else acc[0] += (double)focal(x[e], t[e], alpha, s);
        }
        if (BWD) *reinterpret_cast<f32x4*>(grad + base + t0) = g;
      }
    } else {
      for (int k = lane; k < T; k += 64) {
        float g = 0.f;
        if (counted(mask, mask_kind, mbase + k)) {
          const float x = logits[base + k], t = tgt ? tgt[k] : 0.f;
          const Sig s = sig(x);
          if (BWD) g = scale * focal_grad(x, t, alpha, s);
          else acc[0] += (double)focal(x, t, alpha, s);
        }
        if (BWD) grad[base + k] = g;
      }
    }
  }
  if (!BWD) {
    wave_ops::block_sum<1, kWaves>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
  }
}

// out[0] = the sum of part[0 .. count) in a fixed order
__global__ void __launch_bounds__(kThreads) token_finish(const double* __restrict__ part, int count, float* __restrict__ out) {
  __shared__ double red[kWaves][1];
  double acc[1] = {0.0};
  for (int k = threadIdx.x; k < count; k += kThreads) acc[0] += part[k];
  wave_ops::block_sum<1, kWaves>(acc, red);
  if (threadIdx.x == 0) out[0] = (float)acc[0];
}

// ---- mask losses ---------------------------------------------------------------------------------------------------------------
struct MaskGeom {
  int F, h, w, R, H_im, W_im, stride, start, slices;
  long long P, chunk;        // pixels of an instance (F h w); pixels of a slice, a multiple of 4
};

// the byte of pixel e (= (f h + y) w + x) of an instance whose first row is r0; rows outside [0, R) read as 0
__device__ __forceinline__ const unsigned char* gt_pixel(const unsigned char* __restrict__ gt, const MaskGeom& g, int r0, long long e) {
  const int x = (int)(e % g.w);
  const long long fy = e / g.w;
  const int y = (int)(fy % g.h), f = (int)(fy / g.h);
  return gt + ((long long)(r0 + f) * g.H_im + (g.start + (long long)g.stride * y)) * g.W_im + g.start + (long long)g.stride * x;
}

// VEC: w % 4 == 0 and a 16-byte aligned src: a thread takes 4 pixels of one row.  BWD writes grad_src instead of summing.
template <bool VEC, bool BWD>
__global__ void __launch_bounds__(kThreads)
mask_losses(const float* __restrict__ src, const unsigned char* __restrict__ gt, const int* __restrict__ gt_row, MaskGeom g,
            const float* __restrict__ sums, const float* __restrict__ g_mask_ptr, const float* __restrict__ g_dice_ptr,
            float num_boxes, double* __restrict__ part, float* __restrict__ grad) {
  __shared__ double red[kWaves][4];
  const int i = blockIdx.x / g.slices, sl = blockIdx.x % g.slices;
  const long long lo = sl * g.chunk, hi = min(lo + g.chunk, g.P);
  const int r0 = gt_row[i];
  const bool row_ok = r0 >= 0 && r0 <= g.R - g.F;
  const float* __restrict__ x_i = src + (long long)i * g.P;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  float cf = 0.f, ca = 0.f, cb = 0.f;          // backward: grad = cf focal' + (ca - cb t) sigma'
  if (BWD) {
    const float I = sums[4 * i + 1], den = (sums[4 * i + 2] + sums[4 * i + 3]) + 1.f;
    const float gd = *g_dice_ptr / num_boxes;
    cf = *g_mask_ptr / ((float)g.P * num_boxes);
    ca = gd * (2.f * I + 1.f) / (den * den);
    cb = gd * 2.f / den;
  }
  constexpr int V = VEC ? 4 : 1;
  for (long long e = lo + (long long)threadIdx.x * V; e < hi; e += kThreads * V) {
    float x[V], t[V], out[V];
    if (VEC) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x_i + e);
#pragma unroll
      for (int k = 0; k < V; ++k) x[k] = v[k];
    } else {
      x[0] = x_i[e];
    }
    const unsigned char* __restrict__ b = gt_pixel(gt, g, r0, e);   // VEC: e % 4 == 0 and w % 4 == 0: the 4 pixels share a row
#pragma unroll
    for (int k = 0; k < V; ++k) t[k] = row_ok && b[(long long)k * g.stride] ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const Sig s = sig(x[k]);
      if (BWD) {
        out[k] = cf * focal_grad(x[k], t[k], 0.25f, s) + (ca - cb * t[k]) * (s.p * s.q);
      } else {
        acc[0] += (double)focal(x[k], t[k], 0.25f, s);
        acc[1] += (double)(s.p * t[k]);
        acc[2] += (double)s.p;
        acc[3] += (double)t[k];
      }
    }
    if (BWD) {
      if (VEC) *reinterpret_cast<f32x4*>(grad + (long long)i * g.P + e) = f32x4{out[0], out[V > 1 ? 1 : 0], out[V > 2 ? 2 : 0], out[V > 3 ? 3 : 0]};
      else grad[(long long)i * g.P + e] = out[0];
    }
  }
  if (!BWD) {
    wave_ops::block_sum<4, kWaves>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) part[(long long)blockIdx.x * 4 + k] = acc[k];
    }
  }
}

// sums[i] = the slices of instance i added in a fixed order: a wave per instance, lane l adds slices l, l + 64, ... and the
// wave's butterfly adds the lanes (n = 1 with 2048 slices is 32 loads a lane, not 2048 dependent ones on one thread);
// losses = (loss_mask, loss_dice) added over the instances in a fixed order: per wave in index order, then wave 0..3
__global__ void __launch_bounds__(kThreads)
mask_finish(const double* __restrict__ part, int n, int slices, long long P, float num_boxes, float* __restrict__ sums,
            float* __restrict__ losses) {
  __shared__ double red[kWaves][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double acc[2] = {0.0, 0.0};                  // lane 0 of every wave carries the wave's instances
  for (int i = wv; i < n; i += kWaves) {       // wave-uniform
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int sl = lane; sl < slices; sl += 64) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += part[((long long)i * slices + sl) * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = msda::wave_sum(s[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sums[4 * i + k] = (float)s[k];
      acc[0] += s[0] / (double)P;
      acc[1] += 1.0 - (2.0 * s[1] + 1.0) / (s[2] + s[3] + 1.0);
    }
  }
  wave_ops::block_sum<2, kWaves>(acc, red);
  if (threadIdx.x == 0) {
    losses[0] = (float)(acc[0] / (double)num_boxes);
    losses[1] = (float)(acc[1] / (double)num_boxes);
  }
}

// Pixel slices of an instance: enough for about kTargetBlocks workgroups, none below kMinSlice pixels.  The launcher rounds a
// slice up to a multiple of 4 pixels, so the last slices of a very long instance may start at or past P: their loop does not
// run and they store zero partial sums, on purpose (every partial of the workspace is written on every call).
inline int mask_slices(long long n, long long P) {
  const long long want = msda::ceil_div<long long>(kTargetBlocks, n), most = msda::ceil_div<long long>(P, kMinSlice);
  return (int)(want < most ? want : most);
}

}  // namespace criterion

size_t boxinst_workspace_bytes(long long n, long long P);   // boxinst.hip
const char* g_criterion_last = "";                          // boxinst.hip records its kernels here too

extern "C" {


const char* criterion_hip_last_kernel(void) { return g_criterion_last; }

size_t criterion_hip_workspace_bytes(int which, long long count, long long per) {
  if (count <= 0 || per <= 0) return 0;
  if (which == CRITERION_TOKEN_FOCAL) return (size_t)msda::ceil_div<long long>(count, criterion::kWaves) * sizeof(double);
  if (which == CRITERION_MASK_LOSSES) return (size_t)count * criterion::mask_slices(count, per) * 4 * sizeof(double);
  if (which == CRITERION_BOXINST) return boxinst_workspace_bytes(count, per);
  return 0;
}

static int token_args(const char* who, const float* logits, const void* text_mask, int mask_kind, const int32_t* row_target,
                      const float* positive_map_all, int G, int batch, int Q, int T) {
  if (batch < 0 || Q < 0 || T <= 0 || G < 0) return msda::set_error(DYNMASK_ERR_BAD_DIMS, who);
  if (T > criterion::kMaxT) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "criterion_token_focal: at most 256 tokens");
  if (mask_kind != CRITERION_MASK_NONE && mask_kind != CRITERION_MASK_INT64 && mask_kind != CRITERION_MASK_BOOL)
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "criterion_token_focal: unknown mask kind");
  if ((long long)batch * Q * T >= (1ll << 31)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_token_focal: problem too large");
  if ((long long)batch * Q == 0) return 0;
  if (!logits || !row_target || (G > 0 && !positive_map_all) || (mask_kind != CRITERION_MASK_NONE && !text_mask))
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_token_focal: null pointer argument");
  return 0;
}

int criterion_hip_token_focal_forward_f32(const float* logits, const void* text_mask, int mask_kind, const int32_t* row_target,
                                      const float* positive_map_all, int G, float alpha, int batch, int Q, int T, float* loss,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  if (const int e = token_args("criterion_token_focal_forward: bad dimensions", logits, text_mask, mask_kind, row_target,
                               positive_map_all, G, batch, Q, T))
    return e;
  if (!loss) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_token_focal_forward: null pointer argument");
  const int rows = batch * Q;
  if (rows == 0) return msda::launch_status((int)hipMemsetAsync(loss, 0, sizeof(float), (hipStream_t)stream));
  if (!workspace || workspace_bytes < criterion_hip_workspace_bytes(CRITERION_TOKEN_FOCAL, rows, T) || !msda::aligned16({workspace}))
    return msda::set_error(CRITERION_ERR_WORKSPACE, "criterion_token_focal_forward: workspace too small or not 16-byte aligned");
  const bool vec = T % 4 == 0 && msda::aligned16({logits, positive_map_all});
  const int blocks = msda::ceil_div(rows, criterion::kWaves);
  double* part = static_cast<double*>(workspace);
  auto kernel = vec ? criterion::token_focal<true, false> : criterion::token_focal<false, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(criterion::kThreads), 0, (hipStream_t)stream, logits, text_mask, mask_kind,
                     row_target, positive_map_all, G, alpha, rows, Q, T, (const float*)nullptr, part, (float*)nullptr);
  hipLaunchKernelGGL(criterion::token_finish, dim3(1), dim3(criterion::kThreads), 0, (hipStream_t)stream, part, blocks, loss);
  if (const int e = msda::launch_status()) return e;
  g_criterion_last = vec ? "token_focal_fwd<vec4>" : "token_focal_fwd<scalar>";
  return 0;
}

int criterion_hip_token_focal_backward_f32(const float* logits, const void* text_mask, int mask_kind, const int32_t* row_target,
                                       const float* positive_map_all, int G, float alpha, const float* scale, int batch, int Q,
                                       int T, float* grad_logits, void* stream) {
  if (const int e = token_args("criterion_token_focal_backward: bad dimensions", logits, text_mask, mask_kind, row_target,
                               positive_map_all, G, batch, Q, T))
    return e;
  const int rows = batch * Q;
  if (rows == 0) return 0;
  if (!scale || !grad_logits) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_token_focal_backward: null pointer argument");
  const bool vec = T % 4 == 0 && msda::aligned16({logits, positive_map_all, grad_logits});
  const int blocks = msda::ceil_div(rows, criterion::kWaves);
  auto kernel = vec ? criterion::token_focal<true, true> : criterion::token_focal<false, true>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(criterion::kThreads), 0, (hipStream_t)stream, logits, text_mask, mask_kind,
                     row_target, positive_map_all, G, alpha, rows, Q, T, scale, (double*)nullptr, grad_logits);
  if (const int e = msda::launch_status()) return e;
  g_criterion_last = vec ? "token_focal_bwd<vec4>" : "token_focal_bwd<scalar>";
  return 0;
}

// 0 with `g` filled, 1 for an empty problem, or an error code
static int mask_args(const char* who, const float* src, const unsigned char* gt, const int32_t* gt_row, int n, int F, int h, int w,
                     int R, int H_im, int W_im, int stride, float num_boxes, criterion::MaskGeom* g) {
  if (n < 0 || F <= 0 || h <= 0 || w <= 0 || R < 0 || H_im <= 0 || W_im <= 0 || stride <= 0 || !(num_boxes > 0.f))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, who);
  const int start = stride / 2;
  if (start + (long long)stride * (h - 1) >= H_im || start + (long long)stride * (w - 1) >= W_im)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_mask_losses: the strided pixels do not fit the ground-truth masks");
  const long long P = (long long)F * h * w;
  if (P >= (1ll << 31) || (long long)n * P >= (1ll << 40) || (long long)R * H_im * W_im >= (1ll << 40))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_mask_losses: problem too large");
  if (n == 0) return 1;
  if (!src || !gt || !gt_row) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_mask_losses: null pointer argument");
  const int slices = criterion::mask_slices(n, P);
  if ((long long)n * slices >= (1ll << 31)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_mask_losses: problem too large");
  const long long chunk = msda::round_up<long long>(msda::ceil_div<long long>(P, slices), 4);
  *g = criterion::MaskGeom{F, h, w, R, H_im, W_im, stride, start, slices, P, chunk};
  return 0;
}

int criterion_hip_mask_losses_forward_f32(const float* src, const unsigned char* gt, const int32_t* gt_row, int n, int F, int h, int w,
                                      int R, int H_im, int W_im, int stride, float num_boxes, float* sums, float* losses,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  criterion::MaskGeom g;
  const int e = mask_args("criterion_mask_losses_forward: bad dimensions", src, gt, gt_row, n, F, h, w, R, H_im, W_im, stride,
                          num_boxes, &g);
  if (e < 0 || e > 1) return e;
  if (!losses) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_mask_losses_forward: null pointer argument");
  if (e == 1) return msda::launch_status((int)hipMemsetAsync(losses, 0, 2 * sizeof(float), (hipStream_t)stream));
  if (!sums) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_mask_losses_forward: null pointer argument");
  if (!workspace || workspace_bytes < criterion_hip_workspace_bytes(CRITERION_MASK_LOSSES, n, g.P) || !msda::aligned16({workspace}))
    return msda::set_error(CRITERION_ERR_WORKSPACE, "criterion_mask_losses_forward: workspace too small or not 16-byte aligned");
  const bool vec = w % 4 == 0 && msda::aligned16({src});
  double* part = static_cast<double*>(workspace);
  auto kernel = vec ? criterion::mask_losses<true, false> : criterion::mask_losses<false, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(n * g.slices)), dim3(criterion::kThreads), 0, (hipStream_t)stream, src, gt, gt_row, g,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, num_boxes, part, (float*)nullptr);
  hipLaunchKernelGGL(criterion::mask_finish, dim3(1), dim3(criterion::kThreads), 0, (hipStream_t)stream, part, n, g.slices, g.P,
                     num_boxes, sums, losses);
  if (const int rc = msda::launch_status()) return rc;
  g_criterion_last = vec ? "mask_losses_fwd<vec4>" : "mask_losses_fwd<scalar>";
  return 0;
}

int criterion_hip_mask_losses_backward_f32(const float* src, const unsigned char* gt, const int32_t* gt_row, const float* sums,
                                       const float* grad_mask, const float* grad_dice, int n, int F, int h, int w, int R, int H_im,
                                       int W_im, int stride, float num_boxes, float* grad_src, void* stream) {
  criterion::MaskGeom g;
  const int e = mask_args("criterion_mask_losses_backward: bad dimensions", src, gt, gt_row, n, F, h, w, R, H_im, W_im, stride,
                          num_boxes, &g);
  if (e < 0 || e > 1) return e;
  if (e == 1) return 0;
  if (!sums || !grad_mask || !grad_dice || !grad_src)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_mask_losses_backward: null pointer argument");
  const bool vec = w % 4 == 0 && msda::aligned16({src, grad_src});
  auto kernel = vec ? criterion::mask_losses<true, true> : criterion::mask_losses<false, true>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(n * g.slices)), dim3(criterion::kThreads), 0, (hipStream_t)stream, src, gt, gt_row, g, sums,
                     grad_mask, grad_dice, num_boxes, (double*)nullptr, grad_src);
  if (const int rc = msda::launch_status()) return rc;
  g_criterion_last = vec ? "mask_losses_bwd<vec4>" : "mask_losses_bwd<scalar>";
  return 0;
}

}  // extern "C"
