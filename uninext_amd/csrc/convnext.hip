// ConvNeXt block head / tail and the channels-first LayerNorm -- see include/patch_embed_hip.h.
//
// Three memory-bound kernels, exact fp32, no atomics, every sum in an order fixed by the shape alone.
//
// dwconv_ln<TW>   one 256-thread workgroup owns a th x TW tile of pixels (th <= 8) and walks the channels 32 at a time.  Per
//                 chunk the (th + 6) x (TW + 6) halo of each channel and its 49 weights are staged in LDS (zero padding is
//                 written as zeros).  Lane = channel of the chunk, lane group = tile row: a thread holds its channel's 49
//                 weights in registers, slides a (TW + 6)-wide row of the halo through registers per kernel row and forms its TW
//                 outputs as fmaf chains (bias first, taps in (ky, kx) order).  The per-channel stride of the halo is odd, so
//                 the 32 channels of a half wave read 32 different banks.  The outputs are parked in an LDS plane [pixel][C];
//                 the loads of the next chunk are in flight (in registers) while a chunk is computed.  After the last chunk one
//                 wave per pixel takes the mean and then the sum of squared deviations over the plane (two passes, fixed
//                 order) and writes the normalised row as 16-byte stores.  The convolution output never reaches global memory.
// scale_residual  a 64 x 64 transpose through LDS per (pixel block, channel block, image): the NHWC read runs along C, the NCHW
//                 read of `input` and the write along the pixels.  __fmul_rn / __fadd_rn: two roundings, never an FMA.
//                 scale_residual_drop is the same body with stochastic depth's per-sample factor as a third rounding.
// layernorm_cf    a 1024-thread workgroup owns PX consecutive pixels of one image (lanes along H*W) and splits the channels
//                 over 1024 / PX parts.  The column block is kept in LDS when it fits (one read of x), the partial sums of
//                 the parts are added in part order.
#include "../../include/patch_embed_hip.h"

#include "convnext_common.hpp"

namespace convnext {

template <int TW>
__global__ void __launch_bounds__(kThreads)
dwconv_ln(const float* __restrict__ x, const float* __restrict__ dw_w, const float* __restrict__ dw_b,
          const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps, int C, int H, int W, int th,
          int tiles_x, int tiles_y, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* plane = reinterpret_cast<float*>(smem);                // [th * TW][C]
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tx = bid % tiles_x;
  bid /= tiles_x;
  const int ty = bid % tiles_y, b = bid / tiles_y;
  const int x0 = tx * TW, y0 = ty * th;
  dwconv_to_plane<TW>(x, dw_w, dw_b, C, H, W, th, b, y0, x0, smem);   // convnext_common.hpp

  // LayerNorm over C, one wave per pixel
  const int lane = tid & 63, wave = tid >> 6;
  const int nvec = C >> 2;
  const float inv_c = 1.f / (float)C;
  const f32x4* gv = reinterpret_cast<const f32x4*>(ln_w);
  const f32x4* bv = reinterpret_cast<const f32x4*>(ln_b);
  for (int p = wave; p < th * TW; p += kThreads / 64) {
    const int pr = p / TW, pj = p - pr * TW;
    const int gy = y0 + pr, gx = x0 + pj;
    if (gy >= H || gx >= W) continue;                           // wave-uniform
    const f32x4* pv = reinterpret_cast<const f32x4*>(plane + (size_t)p * C);
    float mean, rstd;
    pixel_stats(pv, nvec, lane, inv_c, eps, mean, rstd);
    f32x4* orow = reinterpret_cast<f32x4*>(out + (((size_t)b * H + gy) * W + gx) * C);
    for (int i = lane; i < nvec; i += 64) {
      const f32x4 v = pv[i], g = gv[i], bb = bv[i];
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (v[e] - mean) * rstd * g[e] + bb[e];
      orow[i] = o;
    }
  }
}

// out[b, c, p] = input[b, c, p] + gamma[c] * y[b, p, c], p over H * W; scale_residual_drop: (gamma[c] * y[b, p, c]) * s[b]
__global__ void __launch_bounds__(kThreads)
scale_residual(const float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ input, int C, int HW,
               float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  scale_residual_body<false>(y, gamma, nullptr, input, C, HW, out, smem);
}
__global__ void __launch_bounds__(kThreads)
scale_residual_drop(const float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ sample_scale,
                    const float* __restrict__ input, int C, int HW, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  scale_residual_body<true>(y, gamma, sample_scale, input, C, HW, out, smem);
}

// channels-first LayerNorm: u = sum_c x / C, s = sum_c (x - u)^2 / C, out = weight * ((x - u) / sqrt(s + eps)) + bias
constexpr int kLnThreads = 1024;
template <bool CACHED>
__global__ void __launch_bounds__(kLnThreads)
layernorm_cf(const float* __restrict__ x, const float* __restrict__ weight, const float* __restrict__ bias, float eps, int C,
             int HW, int px_log2, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int PX = 1 << px_log2, parts = kLnThreads >> px_log2;
  float* red = reinterpret_cast<float*>(smem);                  // [parts][PX]
  float* cache = red + kLnThreads;                              // [C][PX] when CACHED
  const int px = threadIdx.x & (PX - 1), part = threadIdx.x >> px_log2;
  const int p = blockIdx.x * PX + px;
  const bool live = p < HW;
  const size_t img = (size_t)blockIdx.y * C * HW;
  const float* xp = x + img + p;
  float* op = out + img + p;

  float sum = 0.f;
  if (live)
    for (int c = part; c < C; c += parts) {
      const float v = xp[(size_t)c * HW];
      if (CACHED) cache[c * PX + px] = v;
      sum += v;
    }
  red[part * PX + px] = sum;
  __syncthreads();
  float tot = 0.f;
  for (int k = 0; k < parts; ++k) tot += red[k * PX + px];
  const float u = tot / (float)C;
  __syncthreads();
  float sq = 0.f;
  if (live)
    for (int c = part; c < C; c += parts) {
      const float d = (CACHED ? cache[c * PX + px] : xp[(size_t)c * HW]) - u;
      sq += d * d;
    }
  red[part * PX + px] = sq;
  __syncthreads();
  tot = 0.f;
  for (int k = 0; k < parts; ++k) tot += red[k * PX + px];
  const float sd = sqrtf(tot / (float)C + eps);
  if (live)
    for (int c = part; c < C; c += parts) {
      const float v = CACHED ? cache[c * PX + px] : xp[(size_t)c * HW];
      op[(size_t)c * HW] = weight[c] * ((v - u) / sd) + bias[c];
    }
}

static const char* g_last = "";
void set_last_kernel(const char* name) { g_last = name; }

}  // namespace convnext

extern "C" {

const char* patch_embed_hip_convnext_last_kernel(void) { return convnext::g_last; }

int patch_embed_hip_convnext_dwconv_ln_f32(const float* x, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                               const float* ln_bias, float eps, int B, int C, int H, int W, float* out, void* stream) {
  using namespace convnext;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_dwconv_ln: bad dimensions");
  if (C % kChunk != 0 || C > 1536)
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "convnext_dwconv_ln: C must be a multiple of 32, 32 <= C <= 1536");
  if (too_large(B, C, H, W)) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_dwconv_ln: problem too large");
  if (!x || !dw_weight || !ln_weight || !ln_bias || !out)
    return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "convnext_dwconv_ln: null pointer argument");
  if (!msda::aligned16({out, ln_weight, ln_bias}))
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "convnext_dwconv_ln: out, ln_weight and ln_bias must be 16-byte aligned");
  const Tile t = choose_tile(B, C, H, W);
  const int tiles_x = msda::ceil_div(W, t.tw), tiles_y = msda::ceil_div(H, t.th);
  const long long wgs = (long long)B * tiles_x * tiles_y;
  if (t.th == 0 || wgs >= (1ll << 24))   // grid.x * 256 threads stays below 2^32
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_dwconv_ln: problem too large");
  if (B == 0) return 0;
  const int bytes = (int)dwconv_lds_bytes(C, t.th, t.tw);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define CONVNEXT_LAUNCH(TW_)                                                                                                    \
  do {                                                                                                                          \
    static std::atomic<uint64_t> done{0};                                                                                       \
    const int rc = msda::ensure_dynamic_lds(reinterpret_cast<const void*>(&dwconv_ln<TW_>), kLdsBytes, done);                   \
    if (rc) return msda::set_error(rc, "convnext_dwconv_ln: cannot reserve LDS");                                               \
    hipLaunchKernelGGL((dwconv_ln<TW_>), dim3((unsigned)wgs), dim3(kThreads), bytes, st, x, dw_weight, dw_bias, ln_weight,      \
                       ln_bias, eps, C, H, W, t.th, tiles_x, tiles_y, out);                                                     \
    set_last_kernel("convnext_dwconv_ln<" #TW_ ">");                                                                           \
  } while (0)
  if (t.tw == 4) CONVNEXT_LAUNCH(4);
  else if (t.tw == 7) CONVNEXT_LAUNCH(7);
  else CONVNEXT_LAUNCH(8);
#undef CONVNEXT_LAUNCH
  return msda::launch_status();
}

int patch_embed_hip_convnext_scale_residual_f32(const float* y, const float* gamma, const float* input, int B, int C, int H, int W,
                                    float* out, void* stream) {
  using namespace convnext;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_scale_residual: bad dimensions");
  if (too_large(B, C, H, W) || msda::ceil_div(C, kT) > 65535)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_scale_residual: problem too large");
  if (!y || !input || !out) return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "convnext_scale_residual: null pointer argument");
  if (B == 0) return 0;
  const int HW = H * W;
  const dim3 grid((unsigned)msda::ceil_div(HW, kT), (unsigned)msda::ceil_div(C, kT), (unsigned)B);
  hipLaunchKernelGGL(scale_residual, grid, dim3(kThreads), kT * (kT + 1) * sizeof(float), static_cast<hipStream_t>(stream), y,
                     gamma, input, C, HW, out);
  set_last_kernel("convnext_scale_residual");
  return msda::launch_status();
}

int patch_embed_hip_convnext_scale_residual_drop_f32(const float* y, const float* gamma, const float* sample_scale, const float* input,
                                                     int B, int C, int H, int W, float* out, void* stream) {
  using namespace convnext;
  if (!sample_scale) return patch_embed_hip_convnext_scale_residual_f32(y, gamma, input, B, C, H, W, out, stream);
  if (B < 0 || C <= 0 || H <= 0 || W <= 0)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_scale_residual_drop: bad dimensions");
  if (too_large(B, C, H, W) || msda::ceil_div(C, kT) > 65535)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_scale_residual_drop: problem too large");
  if (!y || !input || !out) return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "convnext_scale_residual_drop: null pointer argument");
  if (B == 0) return 0;
  const int HW = H * W;
  const dim3 grid((unsigned)msda::ceil_div(HW, kT), (unsigned)msda::ceil_div(C, kT), (unsigned)B);
  hipLaunchKernelGGL(scale_residual_drop, grid, dim3(kThreads), kT * (kT + 1) * sizeof(float), static_cast<hipStream_t>(stream), y,
                     gamma, sample_scale, input, C, HW, out);
  set_last_kernel("convnext_scale_residual_drop");
  return msda::launch_status();
}

int patch_embed_hip_layernorm_cf_f32(const float* x, const float* weight, const float* bias, float eps, int B, int C, int H, int W,
                         float* out, void* stream) {
  using namespace convnext;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "layernorm_cf: bad dimensions");
  if (too_large(B, C, H, W)) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "layernorm_cf: problem too large");
  if (!x || !weight || !bias || !out) return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "layernorm_cf: null pointer argument");
  if (B == 0) return 0;
  const int HW = H * W;
  // pixels per workgroup: 64 while the [C][PX] block stays inside 128 KiB of LDS, then 32, then 16; past that (C > 2048) x is read
  // three times (from the caches) instead of once, 64 pixels per workgroup again
  const size_t budget = 128 * 1024;
  int px_log2 = 6;
  while (px_log2 > 4 && ((size_t)C << px_log2) * sizeof(float) > budget) --px_log2;
  const bool cached = ((size_t)C << px_log2) * sizeof(float) <= budget;
  if (!cached) px_log2 = 6;   // nothing in LDS bounds the streamed kernel: full 256-byte runs per channel
  const int PX = 1 << px_log2;
  const dim3 grid((unsigned)msda::ceil_div(HW, PX), (unsigned)B);
  const int bytes = (int)((kLnThreads + (cached ? ((size_t)C << px_log2) : 0)) * sizeof(float));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (cached) {
    static std::atomic<uint64_t> done{0};
    const int rc = msda::ensure_dynamic_lds(reinterpret_cast<const void*>(&layernorm_cf<true>), kLdsBytes, done);
    if (rc) return msda::set_error(rc, "layernorm_cf: cannot reserve LDS");
    hipLaunchKernelGGL((layernorm_cf<true>), grid, dim3(kLnThreads), bytes, st, x, weight, bias, eps, C, HW, px_log2, out);
    set_last_kernel("layernorm_cf<cached>");
  } else {
    hipLaunchKernelGGL((layernorm_cf<false>), grid, dim3(kLnThreads), bytes, st, x, weight, bias, eps, C, HW, px_log2, out);
    set_last_kernel("layernorm_cf<streamed>");
  }
  return msda::launch_status();
}

}  // extern "C"
