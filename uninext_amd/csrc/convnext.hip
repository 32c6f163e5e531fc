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
// layernorm_cf    a 1024-thread workgroup owns PX consecutive pixels of one image (lanes along H*W) and splits the channels
//                 over 1024 / PX parts.  The column block is kept in LDS when it fits (one read of x), the partial sums of
//                 the parts are added in part order.
#include "../../include/patch_embed_hip.h"

#include "launch_glue.hpp"
#include "msda_common.hpp"

namespace convnext {

using msda::f32x4;

constexpr int kThreads = 256;
constexpr int kChunk = 32;          // channels per LDS stage: one half wave
constexpr int kMaxTh = 8;           // tile rows: one per group of 32 threads
constexpr int kTaps = 49;
constexpr int kLdsBytes = 160 * 1024;

__host__ __device__ constexpr int halo_stride(int th, int tw) { return ((th + 6) * (tw + 6)) | 1; }

inline size_t dwconv_lds_bytes(int C, int th, int tw) {
  return ((size_t)th * tw * C + (size_t)kChunk * halo_stride(th, tw) + (size_t)kChunk * kTaps + 3) / 4 * 4 * sizeof(float);
}

template <int TW>
__global__ void __launch_bounds__(kThreads)
dwconv_ln(const float* __restrict__ x, const float* __restrict__ dw_w, const float* __restrict__ dw_b,
          const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps, int C, int H, int W, int th,
          int tiles_x, int tiles_y, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int HWD = TW + 6;                                   // halo width
  constexpr int NPRE = (kChunk * (kMaxTh + 6) * HWD + kThreads - 1) / kThreads;
  constexpr int NWPRE = (kChunk * kTaps + kThreads - 1) / kThreads;
  const int hs_raw = (th + 6) * HWD, HS = hs_raw | 1;
  float* plane = reinterpret_cast<float*>(smem);                // [th * TW][C]
  float* halo = plane + (size_t)th * TW * C;                    // [32][HS]
  float* wl = halo + kChunk * HS;                               // [32][49]

  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tx = bid % tiles_x;
  bid /= tiles_x;
  const int ty = bid % tiles_y, b = bid / tiles_y;
  const int x0 = tx * TW, y0 = ty * th;
  const int HW = H * W;

  // where this thread's share of a chunk's halo lives: the same for every chunk
  int goff[NPRE], loff[NPRE];
  const int nh = kChunk * hs_raw;
#pragma unroll
  for (int k = 0; k < NPRE; ++k) {
    const int idx = tid + k * kThreads;
    goff[k] = -1;
    loff[k] = -1;
    if (idx < nh) {
      const int c = idx / hs_raw, rem = idx - c * hs_raw;
      const int hy = rem / HWD, hx = rem - hy * HWD;
      const int gy = y0 - 3 + hy, gx = x0 - 3 + hx;
      loff[k] = c * HS + rem;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) goff[k] = c * HW + gy * W + gx;
    }
  }

  float pre[NPRE], wpre[NWPRE];
  const float* xb = x + (size_t)b * C * HW;
  auto fetch = [&](int cbase) {
    const float* xc = xb + (size_t)cbase * HW;
#pragma unroll
    for (int k = 0; k < NPRE; ++k) pre[k] = goff[k] >= 0 ? xc[goff[k]] : 0.f;
    const float* wc = dw_w + (size_t)cbase * kTaps;
#pragma unroll
    for (int k = 0; k < NWPRE; ++k) {
      const int idx = tid + k * kThreads;
      wpre[k] = idx < kChunk * kTaps ? wc[idx] : 0.f;
    }
  };

  const int c = tid & (kChunk - 1), r = tid >> 5;               // channel of the chunk, tile row
  fetch(0);
  for (int cbase = 0; cbase < C; cbase += kChunk) {
#pragma unroll
    for (int k = 0; k < NPRE; ++k)
      if (loff[k] >= 0) halo[loff[k]] = pre[k];
#pragma unroll
    for (int k = 0; k < NWPRE; ++k) {
      const int idx = tid + k * kThreads;
      if (idx < kChunk * kTaps) wl[idx] = wpre[k];
    }
    __syncthreads();
    if (cbase + kChunk < C) fetch(cbase + kChunk);              // in flight while this chunk is computed
    if (r < th) {
      float w[kTaps];
#pragma unroll
      for (int k = 0; k < kTaps; ++k) w[k] = wl[c * kTaps + k];
      const float bias = dw_b ? dw_b[cbase + c] : 0.f;
      float acc[TW];
#pragma unroll
      for (int j = 0; j < TW; ++j) acc[j] = bias;
      const float* hrow = halo + c * HS + r * HWD;
#pragma unroll
      for (int ky = 0; ky < 7; ++ky) {
        float row[HWD];
#pragma unroll
        for (int i = 0; i < HWD; ++i) row[i] = hrow[ky * HWD + i];
#pragma unroll
        for (int j = 0; j < TW; ++j)
#pragma unroll
          for (int kx = 0; kx < 7; ++kx) acc[j] = fmaf(row[j + kx], w[ky * 7 + kx], acc[j]);
      }
      float* prow = plane + (size_t)(r * TW) * C + cbase + c;
#pragma unroll
      for (int j = 0; j < TW; ++j) prow[(size_t)j * C] = acc[j];
    }
    __syncthreads();
  }

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
    float sum = 0.f;
    for (int i = lane; i < nvec; i += 64) {
      const f32x4 v = pv[i];
      sum += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = msda::wave_sum(sum) * inv_c;
    float sq = 0.f;
    for (int i = lane; i < nvec; i += 64) {
      const f32x4 v = pv[i];
      const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
      sq += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    const float rstd = 1.f / sqrtf(msda::wave_sum(sq) * inv_c + eps);
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

// out[b, c, p] = input[b, c, p] + gamma[c] * y[b, p, c], p over H * W
constexpr int kT = 64;
__global__ void __launch_bounds__(kThreads)
scale_residual(const float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ input, int C, int HW,
               float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = reinterpret_cast<float*>(smem);                 // [64 pixels][65]
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int p0 = blockIdx.x * kT, c0 = blockIdx.y * kT;
  const size_t img = (size_t)blockIdx.z * C * HW;
  const float* yb = y + img;
  const int cin = c0 + lane;
  const float g = (gamma && cin < C) ? gamma[cin] : 1.f;
#pragma unroll 4
  for (int i = grp; i < kT; i += kThreads / 64) {
    const int p = p0 + i;
    if (p < HW && cin < C) {
      const float v = yb[(size_t)p * C + cin];
      tile[i * (kT + 1) + lane] = gamma ? __fmul_rn(g, v) : v;
    }
  }
  __syncthreads();
  const int p = p0 + lane;
#pragma unroll 4
  for (int i = grp; i < kT; i += kThreads / 64) {
    const int cc = c0 + i;
    if (p < HW && cc < C) {
      const size_t o = img + (size_t)cc * HW + p;
      out[o] = __fadd_rn(input[o], tile[lane * (kT + 1) + i]);
    }
  }
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

struct Tile {
  int th, tw;
};

// Tile of the head kernel: a function of the shape alone.  A thread computes one tile row of tw outputs per chunk and the th rows
// of a tile run side by side in the lane groups, so a workgroup's time follows tw and not th: for each width the tile is as tall
// as the LDS plane (and the map) allows, and the width is the one with the least (rounds of workgroups over the 256 CUs, one
// workgroup per CU) x (tw + 2) -- the row's outputs plus the fixed part of a chunk; the wider tile on a tie.
inline Tile choose_tile(int B, int C, int H, int W) {
  const int tws[3] = {4, 7, 8};
  Tile best{0, 0};
  long long best_cost = 0;
  for (int t = 0; t < 3; ++t) {
    const int tw = tws[t];
    int th = H < kMaxTh ? H : kMaxTh;
    while (th > 1 && dwconv_lds_bytes(C, th, tw) > (size_t)kLdsBytes) --th;
    if (dwconv_lds_bytes(C, th, tw) > (size_t)kLdsBytes) continue;
    const long long wgs = (long long)B * ((H + th - 1) / th) * ((W + tw - 1) / tw);
    const long long cost = ((wgs + 255) / 256) * (tw + 2);
    if (best.th == 0 || cost <= best_cost) {
      best = Tile{th, tw};
      best_cost = cost;
    }
  }
  return best;
}

}  // namespace convnext

extern "C" {

static const char* g_convnext_last = "";

const char* patch_embed_hip_convnext_last_kernel(void) { return g_convnext_last; }

static bool convnext_too_large(int B, int C, int H, int W) {
  return (long long)B * C * H * W >= (1ll << 31) || B > 65535 || H > 65535 || W > 65535;   // int offsets, grid.y / grid.z
}


int patch_embed_hip_convnext_dwconv_ln_f32(const float* x, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                               const float* ln_bias, float eps, int B, int C, int H, int W, float* out, void* stream) {
  using namespace convnext;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_dwconv_ln: bad dimensions");
  if (C % kChunk != 0 || C > 1536)
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "convnext_dwconv_ln: C must be a multiple of 32, 32 <= C <= 1536");
  if (convnext_too_large(B, C, H, W)) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_dwconv_ln: problem too large");
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
    g_convnext_last = "convnext_dwconv_ln<" #TW_ ">";                                                                           \
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
  if (convnext_too_large(B, C, H, W) || msda::ceil_div(C, kT) > 65535)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_scale_residual: problem too large");
  if (!y || !input || !out) return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "convnext_scale_residual: null pointer argument");
  if (B == 0) return 0;
  const int HW = H * W;
  const dim3 grid((unsigned)msda::ceil_div(HW, kT), (unsigned)msda::ceil_div(C, kT), (unsigned)B);
  hipLaunchKernelGGL(scale_residual, grid, dim3(kThreads), kT * (kT + 1) * sizeof(float), static_cast<hipStream_t>(stream), y,
                     gamma, input, C, HW, out);
  g_convnext_last = "convnext_scale_residual";
  return msda::launch_status();
}

int patch_embed_hip_layernorm_cf_f32(const float* x, const float* weight, const float* bias, float eps, int B, int C, int H, int W,
                         float* out, void* stream) {
  using namespace convnext;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "layernorm_cf: bad dimensions");
  if (convnext_too_large(B, C, H, W)) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "layernorm_cf: problem too large");
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
    g_convnext_last = "layernorm_cf<cached>";
  } else {
    hipLaunchKernelGGL((layernorm_cf<false>), grid, dim3(kLnThreads), bytes, st, x, weight, bias, eps, C, HW, px_log2, out);
    g_convnext_last = "layernorm_cf<streamed>";
  }
  return msda::launch_status();
}

}  // extern "C"
