// What convnext.hip (forward) and convnext_bwd.hip (training) share: the chunking constants, the tile rule of the block's head,
// the head's convolution stage and its per-pixel statistics (one text, so the backward recomputes the forward's values to the
// bit), and the body of the tail's transpose.  Internal, not part of the C ABI.
#pragma once

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

// The head's convolution stage: the workgroup's th x TW tile at (y0, x0) of image b, all C channels 32 at a time, into the LDS
// plane [th * TW][C] at the start of smem (halo and weights behind it).  Ends with a __syncthreads().
template <int TW>
__device__ __forceinline__ void dwconv_to_plane(const float* __restrict__ x, const float* __restrict__ dw_w,
                                                const float* __restrict__ dw_b, int C, int H, int W, int th, int b, int y0, int x0,
                                                char* smem) {
  constexpr int HWD = TW + 6;                                   // halo width
  constexpr int NPRE = (kChunk * (kMaxTh + 6) * HWD + kThreads - 1) / kThreads;
  constexpr int NWPRE = (kChunk * kTaps + kThreads - 1) / kThreads;
  const int hs_raw = (th + 6) * HWD, HS = hs_raw | 1;
  float* plane = reinterpret_cast<float*>(smem);                // [th * TW][C]
  float* halo = plane + (size_t)th * TW * C;                    // [32][HS]
  float* wl = halo + kChunk * HS;                               // [32][49]

  const int tid = threadIdx.x;
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
}

// Mean and 1 / sqrt(var + eps) of one pixel's C channels in the plane, by one wave: two passes, fixed order.
__device__ __forceinline__ void pixel_stats(const f32x4* pv, int nvec, int lane, float inv_c, float eps, float& mean, float& rstd) {
  float sum = 0.f;
  for (int i = lane; i < nvec; i += 64) {
    const f32x4 v = pv[i];
    sum += (v[0] + v[1]) + (v[2] + v[3]);
  }
  mean = msda::wave_sum(sum) * inv_c;
  float sq = 0.f;
  for (int i = lane; i < nvec; i += 64) {
    const f32x4 v = pv[i];
    const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
    sq += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  rstd = 1.f / sqrtf(msda::wave_sum(sq) * inv_c + eps);
}

// out[b, c, p] = input[b, c, p] + (gamma[c] * y[b, p, c]) * s[b], p over H * W: a 64 x 64 transpose through LDS per (pixel block,
// channel block, image).  Every product and the sum are rounded on their own.  DROP = false: no s.
constexpr int kT = 64;
template <bool DROP>
__device__ __forceinline__ void scale_residual_body(const float* __restrict__ y, const float* __restrict__ gamma,
                                                    const float* __restrict__ sample_scale, const float* __restrict__ input, int C,
                                                    int HW, float* __restrict__ out, char* smem) {
  float* tile = reinterpret_cast<float*>(smem);                 // [64 pixels][65]
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int p0 = blockIdx.x * kT, c0 = blockIdx.y * kT;
  const size_t img = (size_t)blockIdx.z * C * HW;
  const float* yb = y + img;
  const int cin = c0 + lane;
  const float g = (gamma && cin < C) ? gamma[cin] : 1.f;
  const float s = DROP ? sample_scale[blockIdx.z] : 1.f;
#pragma unroll 4
  for (int i = grp; i < kT; i += kThreads / 64) {
    const int p = p0 + i;
    if (p < HW && cin < C) {
      const float v = yb[(size_t)p * C + cin];
      const float gv = gamma ? __fmul_rn(g, v) : v;
      tile[i * (kT + 1) + lane] = DROP ? __fmul_rn(gv, s) : gv;
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

inline bool too_large(int B, int C, int H, int W) {
  return (long long)B * C * H * W >= (1ll << 31) || B > 65535 || H > 65535 || W > 65535;   // int offsets, grid.y / grid.z
}

// the record behind patch_embed_hip_convnext_last_kernel (convnext.hip)
void set_last_kernel(const char* name);

}  // namespace convnext
