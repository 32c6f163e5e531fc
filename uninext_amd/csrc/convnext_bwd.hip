// Backward of the ConvNeXt block head / tail and of the channels-first LayerNorm -- see include/patch_embed_hip.h.
//
// Exact fp32 products, no atomics, every sum in an order fixed by the shape alone.  Sums over pixels: fp32 inside a workgroup (at
// most a tile, a band of 64 tiles or 64 pixels), the workgroups' partial sums in the caller's workspace, added in float64 in
// workgroup order by reduce_partials.
//
// head_bwd_gu<TW>   pass one of the head, on the forward's tiling: dwconv_to_plane and pixel_stats (convnext_common.hpp) recompute
//                   the convolution output u and its statistics to the bit; one wave per pixel then takes mean_C(gw) and
//                   mean_C(gw * xhat), gw = grad_out * ln_weight.  With lane = channel of a chunk and lane group = tile row a
//                   thread forms grad_u = rstd * (gw - mean_C(gw) - xhat * mean_C(gw * xhat)) of its TW pixels, writes it as NCHW
//                   into the workspace and keeps the sums of grad_out and grad_out * xhat; it parks them in the two plane entries
//                   only it has read, and the rows are added in row order: [workgroup][2][C] partials.
// head_bwd_xw       pass two, per (band of 8 x 8 tiles, chunk of 32 channels): the 14 x 14 halos of grad_u and x in LDS (odd
//                   channel stride, zeros outside the map); grad_x as 49-tap fmaf chains over grad_u with the mirrored weights;
//                   the 49 weight sums and the bias sum of (channel, tile row) stay in registers over the band, then the eight
//                   rows are added in row order: [band][C * 49] and [band][C] partials.
// tail_bwd          the 64 x 64 transpose of the forward, the other way round: grad_y = (grad_out * s) * gamma, and the sums of
//                   (grad_out * s) * y over the block's 64 pixels: [image * pixel block][C] partials.
// layernorm_cf_bwd  the forward's layout with 64 pixels per workgroup (one wave = one part of the channels, lanes along H * W): u
//                   and sd by the forward's arithmetic, the two channel means through LDS in part order, grad_x, and per channel
//                   a wave sum over the 64 pixels: [image * pixel block][2][C] partials.  x stays in LDS up to C = 512.
#include "../../include/patch_embed_hip.h"

#include "convnext_common.hpp"

namespace convnext {

// A product rounded on its own.  (__fmul_rn is a plain product to the compiler, which may fuse it into the subtraction that follows;
// gw - mean_C(gw) must see the same gw the mean was taken of: with one channel it is exactly 0.)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// ---- the head, pass one -------------------------------------------------------------------------------------------------------
template <int TW>
__global__ void __launch_bounds__(kThreads)
head_bwd_gu(const float* __restrict__ x, const float* __restrict__ dw_w, const float* __restrict__ dw_b,
            const float* __restrict__ ln_w, float eps, const float* __restrict__ go, int C, int H, int W, int th, int tiles_x,
            int tiles_y, float* __restrict__ gu, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* plane = reinterpret_cast<float*>(smem);                // [th * TW][C]
  float* stat = plane + (size_t)th * TW * C;                    // [th * TW][4] over the halo, which is free after the convolution
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tx = bid % tiles_x;
  bid /= tiles_x;
  const int ty = bid % tiles_y, b = bid / tiles_y;
  const int x0 = tx * TW, y0 = ty * th;
  dwconv_to_plane<TW>(x, dw_w, dw_b, C, H, W, th, b, y0, x0, smem);

  // per pixel, one wave: the forward's mean and rstd, then the two channel means of the LayerNorm backward
  const int lane = tid & 63, wave = tid >> 6;
  const int nvec = C >> 2;
  const float inv_c = 1.f / (float)C;
  const f32x4* wv = reinterpret_cast<const f32x4*>(ln_w);
  for (int p = wave; p < th * TW; p += kThreads / 64) {
    const int pr = p / TW, pj = p - pr * TW;
    const int gy = y0 + pr, gx = x0 + pj;
    if (gy >= H || gx >= W) continue;                           // wave-uniform
    const f32x4* pv = reinterpret_cast<const f32x4*>(plane + (size_t)p * C);
    float mean, rstd;
    pixel_stats(pv, nvec, lane, inv_c, eps, mean, rstd);
    const f32x4* gv = reinterpret_cast<const f32x4*>(go + (((size_t)b * H + gy) * W + gx) * C);
    float s1 = 0.f, s2 = 0.f;
    for (int i = lane; i < nvec; i += 64) {
      const f32x4 v = pv[i], g = gv[i], w = wv[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gw = mul_rn(g[e], w[e]);                      // rounded on its own here and below: the same gw in both
        s1 += gw;
        s2 += gw * ((v[e] - mean) * rstd);
      }
    }
    s1 = msda::wave_sum(s1) * inv_c;
    s2 = msda::wave_sum(s2) * inv_c;
    if (lane == 0) {
      float* st = stat + p * 4;
      st[0] = mean;
      st[1] = rstd;
      st[2] = s1;
      st[3] = s2;
    }
  }
  __syncthreads();

  // lane = channel of the chunk, lane group = tile row
  const int c = tid & (kChunk - 1), r = tid >> 5;
  if (r < th) {
    const int gy = y0 + r;
    for (int cbase = 0; cbase < C; cbase += kChunk) {
      const int ch = cbase + c;
      float sb = 0.f, sw = 0.f;
      if (gy < H) {
        const float lw = ln_w[ch];
        const float* grow = go + (((size_t)b * H + gy) * W + x0) * C + ch;
        float* urow = gu ? gu + (((size_t)b * C + ch) * H + gy) * W + x0 : nullptr;
#pragma unroll
        for (int j = 0; j < TW; ++j) {
          if (x0 + j < W) {
            const int p = r * TW + j;
            const float* st = stat + p * 4;
            const float xh = (plane[(size_t)p * C + ch] - st[0]) * st[1];
            const float g = grow[(size_t)j * C];
            sb += g;
            sw += g * xh;
            if (urow) urow[j] = st[1] * (mul_rn(g, lw) - st[2] - xh * st[3]);
          }
        }
      }
      // the entries (r, j = 0 / 1, ch) of the plane: read by this thread alone, above
      plane[(size_t)(r * TW) * C + ch] = sb;
      plane[(size_t)(r * TW + 1) * C + ch] = sw;
    }
  }
  if (part == nullptr) return;                                  // uniform
  __syncthreads();
  float* pb = part + (size_t)blockIdx.x * 2 * C;
  for (int ch = tid; ch < C; ch += kThreads) {
    float sb = 0.f, sw = 0.f;
    for (int rr = 0; rr < th; ++rr) {
      sb += plane[(size_t)(rr * TW) * C + ch];
      sw += plane[(size_t)(rr * TW + 1) * C + ch];
    }
    pb[ch] = sb;
    pb[C + ch] = sw;
  }
}

// ---- the head, pass two -------------------------------------------------------------------------------------------------------
constexpr int kBT = 8;                                          // tile side of pass two
constexpr int kBH = kBT + 6;                                    // halo side
constexpr int kBHS = halo_stride(kBT, kBT);                     // 197: odd, 32 channels on 32 banks
constexpr int kBandTiles = 64;                                  // most tiles a band sums in fp32
constexpr int kBandTarget = 512;                                // workgroups pass two aims at: two per CU (56 KB of LDS each)
constexpr int kXwLds = kMaxTh * kChunk * (kTaps + 1);           // the closing sum of the eight rows; the two halos are smaller
static_assert(2 * kChunk * kBHS <= kXwLds, "the halos fit");

template <bool DX, bool DW>
__global__ void __launch_bounds__(kThreads)
head_bwd_xw(const float* __restrict__ gu, const float* __restrict__ x, const float* __restrict__ dw_w, int C, int H, int W,
            int tiles_x, int tiles_y, int total_tiles, int tiles_per_band, float* __restrict__ gx, float* __restrict__ pw,
            float* __restrict__ pb) {
  __shared__ float lds[kXwLds];
  __shared__ float wl[kChunk * kTaps];                          // the chunk's weights: in registers they would crowd out the sums
  float* hg = lds;                                              // [32][197] grad_u
  float* hx = lds + kChunk * kBHS;                              // [32][197] x
  const int tid = threadIdx.x;
  const int c = tid & (kChunk - 1), r = tid >> 5;
  const int cbase = blockIdx.y * kChunk;
  const int HW = H * W;
  float aw[kTaps], ab = 0.f;
#pragma unroll
  for (int k = 0; k < kTaps; ++k) aw[k] = 0.f;
  if (DX)
    for (int idx = tid; idx < kChunk * kTaps; idx += kThreads) wl[idx] = dw_w[(size_t)cbase * kTaps + idx];
  const float* w = wl + c * kTaps;                              // read after the first tile's barrier
  const int t0 = blockIdx.x * tiles_per_band;
  const int t1 = t0 + tiles_per_band < total_tiles ? t0 + tiles_per_band : total_tiles;
  for (int t = t0; t < t1; ++t) {
    const int tx = t % tiles_x, q = t / tiles_x;
    const int ty = q % tiles_y, b = q / tiles_y;
    const int x0 = tx * kBT, y0 = ty * kBT;
    const size_t base = ((size_t)b * C + cbase) * HW;
    __syncthreads();                                            // the tile before has been read
    for (int idx = tid; idx < kChunk * kBH * kBH; idx += kThreads) {
      const int cc = idx / (kBH * kBH), rem = idx - cc * (kBH * kBH);
      const int hy = rem / kBH, hxx = rem - hy * kBH;
      const int gy = y0 - 3 + hy, gxx = x0 - 3 + hxx;
      const bool in = gy >= 0 && gy < H && gxx >= 0 && gxx < W;
      const size_t off = base + (size_t)cc * HW + (size_t)gy * W + gxx;
      hg[cc * kBHS + rem] = in ? gu[off] : 0.f;
      if (DW) hx[cc * kBHS + rem] = in ? x[off] : 0.f;
    }
    __syncthreads();
    const float* gr = hg + c * kBHS + r * kBH;
    const float* xr = hx + c * kBHS + r * kBH;
    float acc[kBT], gc[kBT];
#pragma unroll
    for (int j = 0; j < kBT; ++j) {
      acc[j] = 0.f;
      gc[j] = gr[3 * kBH + 3 + j];                              // grad_u of the thread's own pixels (0 outside the map)
      if (DW) ab += gc[j];
    }
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      if (DX) {                                                 // grad_x[h, w] += grad_u[h - 3 + ky, w - 3 + kx] * weight[6 - ky, 6 - kx]
        float row[kBH];
#pragma unroll
        for (int i = 0; i < kBH; ++i) row[i] = gr[ky * kBH + i];
#pragma unroll
        for (int j = 0; j < kBT; ++j)
#pragma unroll
          for (int kx = 0; kx < 7; ++kx) acc[j] = fmaf(row[j + kx], w[(6 - ky) * 7 + (6 - kx)], acc[j]);
      }
      if (DW) {                                                 // grad_weight[ky, kx] += grad_u[h, w] * x[h - 3 + ky, w - 3 + kx]
        float row[kBH];
#pragma unroll
        for (int i = 0; i < kBH; ++i) row[i] = xr[ky * kBH + i];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
#pragma unroll
          for (int j = 0; j < kBT; ++j) aw[ky * 7 + kx] = fmaf(gc[j], row[j + kx], aw[ky * 7 + kx]);
      }
    }
    if (DX) {
      const int gy = y0 + r;
      if (gy < H) {
        float* orow = gx + base + (size_t)c * HW + (size_t)gy * W + x0;
#pragma unroll
        for (int j = 0; j < kBT; ++j)
          if (x0 + j < W) orow[j] = acc[j];
      }
    }
  }
  if (!DW) return;
  __syncthreads();
  float* red = lds;                                             // [8][32][50]
  float* mine = red + (size_t)(r * kChunk + c) * (kTaps + 1);
#pragma unroll
  for (int k = 0; k < kTaps; ++k) mine[k] = aw[k];
  mine[kTaps] = ab;
  __syncthreads();
  for (int idx = tid; idx < kChunk * (kTaps + 1); idx += kThreads) {
    const int cc = idx / (kTaps + 1), k = idx - cc * (kTaps + 1);
    float s = 0.f;
    for (int rr = 0; rr < kMaxTh; ++rr) s += red[(size_t)(rr * kChunk + cc) * (kTaps + 1) + k];
    if (k < kTaps) pw[((size_t)blockIdx.x * C + cbase + cc) * kTaps + k] = s;
    else pb[(size_t)blockIdx.x * C + cbase + cc] = s;
  }
}

// out[col] = sum_i part[i * ld + col] over the n partial rows, in float64: eight interleaved runs, added in run order
__global__ void __launch_bounds__(kThreads)
reduce_partials(const float* __restrict__ part, int n, int ld, int cols, float* __restrict__ out) {
  __shared__ double red[kThreads / kChunk][kChunk];
  const int l = threadIdx.x & (kChunk - 1), g = threadIdx.x >> 5;
  const int col = blockIdx.x * kChunk + l;
  double s = 0.0;
  if (col < cols)
    for (int i = g; i < n; i += kThreads / kChunk) s += (double)part[(size_t)i * ld + col];
  red[g][l] = s;
  __syncthreads();
  if (g == 0 && col < cols) {
    double t = red[0][l];
    for (int k = 1; k < kThreads / kChunk; ++k) t += red[k][l];
    out[col] = (float)t;
  }
}

// ---- the tail -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
tail_bwd(const float* __restrict__ go, const float* __restrict__ y, const float* __restrict__ gamma,
         const float* __restrict__ sample_scale, int C, int HW, float* __restrict__ gy, float* __restrict__ part) {
  __shared__ float tile[kT * (kT + 1)];                         // [64 channels][65]
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int p0 = blockIdx.x * kT, c0 = blockIdx.y * kT;
  const size_t img = (size_t)blockIdx.z * C * HW;
  const float s = sample_scale ? sample_scale[blockIdx.z] : 1.f;
  const int pin = p0 + lane;
#pragma unroll 4
  for (int i = grp; i < kT; i += kThreads / 64) {
    const int cc = c0 + i;
    if (pin < HW && cc < C) {
      const float v = go[img + (size_t)cc * HW + pin];
      tile[i * (kT + 1) + lane] = sample_scale ? __fmul_rn(v, s) : v;
    }
  }
  __syncthreads();
  const int cin = c0 + lane;
  const float g = (gamma && cin < C) ? gamma[cin] : 1.f;
  float acc = 0.f;
#pragma unroll 4
  for (int i = grp; i < kT; i += kThreads / 64) {
    const int p = p0 + i;
    if (p < HW && cin < C) {
      const float t = tile[lane * (kT + 1) + i];
      const size_t o = img + (size_t)p * C + cin;
      if (part) acc = fmaf(t, y[o], acc);
      if (gy) gy[o] = gamma ? __fmul_rn(t, g) : t;
    }
  }
  if (part == nullptr) return;                                  // uniform
  __syncthreads();
  tile[grp * kT + lane] = acc;
  __syncthreads();
  if (grp == 0 && cin < C) {
    float t = tile[lane];
    for (int k = 1; k < kThreads / 64; ++k) t += tile[k * kT + lane];
    part[((size_t)blockIdx.z * gridDim.x + blockIdx.x) * C + cin] = t;
  }
}

// ---- channels-first LayerNorm -----------------------------------------------------------------------------------------------------
constexpr int kLnThreads = 1024;
constexpr int kLnPx = 64;                                       // pixels per workgroup: one wave is one part of the channels
constexpr int kLnParts = kLnThreads / kLnPx;
constexpr int kLnCachedC = 512;                                 // [C][64] floats of x in LDS up to here: 128 KiB

template <bool CACHED>
__global__ void __launch_bounds__(kLnThreads)
layernorm_cf_bwd(const float* __restrict__ x, const float* __restrict__ weight, float eps, const float* __restrict__ go, int C,
                 int HW, float* __restrict__ gx, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);                  // [2][parts][64]
  float* cache = red + 2 * kLnThreads;                          // [C][64] when CACHED
  const int px = threadIdx.x & (kLnPx - 1), pt = threadIdx.x >> 6;
  const int p = blockIdx.x * kLnPx + px;
  const bool live = p < HW;
  const size_t img = (size_t)blockIdx.y * C * HW;
  const float* xp = x + img + p;
  const float* gp = go + img + p;

  // u and sd: the forward's arithmetic
  float sum = 0.f;
  if (live)
    for (int c = pt; c < C; c += kLnParts) {
      const float v = xp[(size_t)c * HW];
      if (CACHED) cache[c * kLnPx + px] = v;
      sum += v;
    }
  red[pt * kLnPx + px] = sum;
  __syncthreads();
  float tot = 0.f;
  for (int k = 0; k < kLnParts; ++k) tot += red[k * kLnPx + px];
  const float u = tot / (float)C;
  __syncthreads();
  float sq = 0.f;
  if (live)
    for (int c = pt; c < C; c += kLnParts) {
      const float d = (CACHED ? cache[c * kLnPx + px] : xp[(size_t)c * HW]) - u;
      sq += d * d;
    }
  red[pt * kLnPx + px] = sq;
  __syncthreads();
  tot = 0.f;
  for (int k = 0; k < kLnParts; ++k) tot += red[k * kLnPx + px];
  const float sd = sqrtf(tot / (float)C + eps);
  __syncthreads();

  // mean_C(gw) and mean_C(gw * xhat), gw = grad_out * weight
  float m1 = 0.f, m2 = 0.f;
  if (gx) {
    float s1 = 0.f, s2 = 0.f;
    if (live)
      for (int c = pt; c < C; c += kLnParts) {
        const float v = CACHED ? cache[c * kLnPx + px] : xp[(size_t)c * HW];
        const float gw = mul_rn(gp[(size_t)c * HW], weight[c]);      // rounded on its own here and below: C = 1 gives exactly 0
        s1 += gw;
        s2 += gw * ((v - u) / sd);
      }
    red[pt * kLnPx + px] = s1;
    red[kLnThreads + pt * kLnPx + px] = s2;
    __syncthreads();
    for (int k = 0; k < kLnParts; ++k) {
      m1 += red[k * kLnPx + px];
      m2 += red[kLnThreads + k * kLnPx + px];
    }
    m1 /= (float)C;
    m2 /= (float)C;
  }

  float* pbase = part ? part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * C : nullptr;
  for (int c = pt; c < C; c += kLnParts) {                      // every lane of the wave: the wave sums below
    float g = 0.f, xh = 0.f;
    if (live) {
      const float v = CACHED ? cache[c * kLnPx + px] : xp[(size_t)c * HW];
      g = gp[(size_t)c * HW];
      xh = (v - u) / sd;
      if (gx) gx[img + (size_t)c * HW + p] = (mul_rn(g, weight[c]) - m1 - xh * m2) / sd;
    }
    if (pbase) {
      const float sb = msda::wave_sum(g), sw = msda::wave_sum(g * xh);
      if (px == 0) {
        pbase[c] = sb;
        pbase[C + c] = sw;
      }
    }
  }
}

// ---- host side: the workspaces -----------------------------------------------------------------------------------------------------
struct Bands {
  int tiles_x, tiles_y, total, per_band, bands;
};

// Bands of pass two: a function of the shape alone.  About kBandTarget workgroups over the C / 32 chunks, at least one tile and at
// most kBandTiles tiles a band.
inline Bands choose_bands(int B, int C, int H, int W) {
  Bands s;
  s.tiles_x = msda::ceil_div(W, kBT);
  s.tiles_y = msda::ceil_div(H, kBT);
  const long long total = (long long)B * s.tiles_x * s.tiles_y;   // < 2^31 / 32 with too_large() passed
  s.total = (int)total;
  const int want = kBandTarget / (C / kChunk) > 1 ? kBandTarget / (C / kChunk) : 1;
  long long per = msda::ceil_div(total, (long long)want);
  if (per > kBandTiles) per = kBandTiles;
  if (per < 1) per = 1;
  s.per_band = (int)per;
  s.bands = (int)msda::ceil_div(total, per);
  return s;
}

struct HeadWorkspace {
  size_t gu, part1, pw, pb, total;                              // offsets in bytes
  Tile tile;
  int tiles_x, tiles_y;
  long long wgs;
  Bands bands;
};

inline bool head_shape_ok(int B, int C, int H, int W) {
  return B >= 0 && C > 0 && H > 0 && W > 0 && C % kChunk == 0 && C <= 1536 && !too_large(B, C, H, W);
}

inline HeadWorkspace head_workspace(int B, int C, int H, int W) {
  HeadWorkspace ws{};
  ws.tile = choose_tile(B, C, H, W);
  ws.tiles_x = msda::ceil_div(W, ws.tile.tw);
  ws.tiles_y = msda::ceil_div(H, ws.tile.th);
  ws.wgs = (long long)B * ws.tiles_x * ws.tiles_y;
  ws.bands = choose_bands(B, C, H, W);
  ws.gu = 0;
  ws.part1 = ws.gu + msda::align256((size_t)B * C * H * W * sizeof(float));
  ws.pw = ws.part1 + msda::align256((size_t)ws.wgs * 2 * C * sizeof(float));
  ws.pb = ws.pw + msda::align256((size_t)ws.bands.bands * C * kTaps * sizeof(float));
  ws.total = ws.pb + msda::align256((size_t)ws.bands.bands * C * sizeof(float));
  return ws;
}

inline int launch_reduce(const float* part, int n, int ld, int cols, float* out, hipStream_t st) {
  hipLaunchKernelGGL(reduce_partials, dim3((unsigned)msda::ceil_div(cols, kChunk)), dim3(kThreads), 0, st, part, n, ld, cols, out);
  return 0;
}

}  // namespace convnext

extern "C" {

size_t patch_embed_hip_convnext_dwconv_ln_backward_workspace_bytes(int B, int C, int H, int W) {
  using namespace convnext;
  if (!head_shape_ok(B, C, H, W) || B == 0) return 0;
  const HeadWorkspace ws = head_workspace(B, C, H, W);
  return (ws.tile.th == 0 || ws.wgs >= (1ll << 24)) ? 0 : ws.total;
}

int patch_embed_hip_convnext_dwconv_ln_backward_f32(const float* x, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                                                    float eps, const float* grad_out, int B, int C, int H, int W, float* grad_x,
                                                    float* grad_dw_weight, float* grad_dw_bias, float* grad_ln_weight,
                                                    float* grad_ln_bias, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace convnext;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_dwconv_ln_backward: bad dimensions");
  if (C % kChunk != 0 || C > 1536)
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "convnext_dwconv_ln_backward: C must be a multiple of 32, 32 <= C <= 1536");
  if (too_large(B, C, H, W)) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_dwconv_ln_backward: problem too large");
  if (!x || !dw_weight || !ln_weight || !grad_out)
    return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "convnext_dwconv_ln_backward: null pointer argument");
  if (!msda::aligned16({grad_out, ln_weight}))
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "convnext_dwconv_ln_backward: grad_out and ln_weight must be 16-byte aligned");
  const HeadWorkspace ws = head_workspace(B, C, H, W);
  if (ws.tile.th == 0 || ws.wgs >= (1ll << 24))   // grid.x * 256 threads stays below 2^32
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_dwconv_ln_backward: problem too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (B == 0) {   // the gradients of a sum over no pixels
    if (grad_dw_weight && hipMemsetAsync(grad_dw_weight, 0, (size_t)C * kTaps * sizeof(float), st) != hipSuccess) return msda::launch_status();
    if (grad_dw_bias && hipMemsetAsync(grad_dw_bias, 0, (size_t)C * sizeof(float), st) != hipSuccess) return msda::launch_status();
    if (grad_ln_weight && hipMemsetAsync(grad_ln_weight, 0, (size_t)C * sizeof(float), st) != hipSuccess) return msda::launch_status();
    if (grad_ln_bias && hipMemsetAsync(grad_ln_bias, 0, (size_t)C * sizeof(float), st) != hipSuccess) return msda::launch_status();
    return 0;
  }
  if (!workspace || workspace_bytes < ws.total)
    return msda::set_error(PATCH_EMBED_ERR_WORKSPACE, "convnext_dwconv_ln_backward: workspace too small");
  const bool two = grad_x || grad_dw_weight || grad_dw_bias, ln = grad_ln_weight || grad_ln_bias;
  if (!two && !ln) return 0;
  char* base = static_cast<char*>(workspace);
  float* gu = reinterpret_cast<float*>(base + ws.gu);
  float* part1 = reinterpret_cast<float*>(base + ws.part1);
  float* pw = reinterpret_cast<float*>(base + ws.pw);
  float* pb = reinterpret_cast<float*>(base + ws.pb);
  const int bytes = (int)dwconv_lds_bytes(C, ws.tile.th, ws.tile.tw);
#define CONVNEXT_LAUNCH(TW_)                                                                                                    \
  do {                                                                                                                          \
    static std::atomic<uint64_t> done{0};                                                                                       \
    const int rc = msda::ensure_dynamic_lds(reinterpret_cast<const void*>(&head_bwd_gu<TW_>), kLdsBytes, done);                 \
    if (rc) return msda::set_error(rc, "convnext_dwconv_ln_backward: cannot reserve LDS");                                      \
    hipLaunchKernelGGL((head_bwd_gu<TW_>), dim3((unsigned)ws.wgs), dim3(kThreads), bytes, st, x, dw_weight, dw_bias, ln_weight, \
                       eps, grad_out, C, H, W, ws.tile.th, ws.tiles_x, ws.tiles_y, two ? gu : nullptr, ln ? part1 : nullptr);   \
    set_last_kernel("convnext_dwconv_ln_backward<" #TW_ ">");                                                                   \
  } while (0)
  if (ws.tile.tw == 4) CONVNEXT_LAUNCH(4);
  else if (ws.tile.tw == 7) CONVNEXT_LAUNCH(7);
  else CONVNEXT_LAUNCH(8);
#undef CONVNEXT_LAUNCH
  if (grad_ln_bias) launch_reduce(part1, (int)ws.wgs, 2 * C, C, grad_ln_bias, st);
  if (grad_ln_weight) launch_reduce(part1 + C, (int)ws.wgs, 2 * C, C, grad_ln_weight, st);
  if (two) {
    const Bands& bd = ws.bands;
    const dim3 grid((unsigned)bd.bands, (unsigned)(C / kChunk));
    const bool dw = grad_dw_weight || grad_dw_bias;
    if (grad_x && dw)
      hipLaunchKernelGGL((head_bwd_xw<true, true>), grid, dim3(kThreads), 0, st, gu, x, dw_weight, C, H, W, bd.tiles_x, bd.tiles_y,
                         bd.total, bd.per_band, grad_x, pw, pb);
    else if (grad_x)
      hipLaunchKernelGGL((head_bwd_xw<true, false>), grid, dim3(kThreads), 0, st, gu, x, dw_weight, C, H, W, bd.tiles_x, bd.tiles_y,
                         bd.total, bd.per_band, grad_x, pw, pb);
    else
      hipLaunchKernelGGL((head_bwd_xw<false, true>), grid, dim3(kThreads), 0, st, gu, x, dw_weight, C, H, W, bd.tiles_x, bd.tiles_y,
                         bd.total, bd.per_band, grad_x, pw, pb);
    if (grad_dw_weight) launch_reduce(pw, bd.bands, C * kTaps, C * kTaps, grad_dw_weight, st);
    if (grad_dw_bias) launch_reduce(pb, bd.bands, C, C, grad_dw_bias, st);
  }
  return msda::launch_status();
}

size_t patch_embed_hip_convnext_scale_residual_backward_workspace_bytes(int B, int C, int H, int W) {
  using namespace convnext;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || too_large(B, C, H, W) || msda::ceil_div(C, kT) > 65535) return 0;
  return msda::align256((size_t)B * msda::ceil_div(H * W, kT) * C * sizeof(float));
}

int patch_embed_hip_convnext_scale_residual_backward_f32(const float* grad_out, const float* y, const float* gamma, const float* sample_scale,
                                                         int B, int C, int H, int W, float* grad_y, float* grad_gamma, void* workspace,
                                                         size_t workspace_bytes, void* stream) {
  using namespace convnext;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_scale_residual_backward: bad dimensions");
  if (too_large(B, C, H, W) || msda::ceil_div(C, kT) > 65535)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "convnext_scale_residual_backward: problem too large");
  if (!grad_out || (grad_gamma && (!y || !gamma)))
    return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "convnext_scale_residual_backward: null pointer argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (B == 0) {
    if (grad_gamma && hipMemsetAsync(grad_gamma, 0, (size_t)C * sizeof(float), st) != hipSuccess) return msda::launch_status();
    return 0;
  }
  const int HW = H * W, nblk = msda::ceil_div(HW, kT);
  if (grad_gamma && (!workspace || workspace_bytes < msda::align256((size_t)B * nblk * C * sizeof(float))))
    return msda::set_error(PATCH_EMBED_ERR_WORKSPACE, "convnext_scale_residual_backward: workspace too small");
  if (!grad_y && !grad_gamma) return 0;
  float* part = grad_gamma ? static_cast<float*>(workspace) : nullptr;
  const dim3 grid((unsigned)nblk, (unsigned)msda::ceil_div(C, kT), (unsigned)B);
  hipLaunchKernelGGL(tail_bwd, grid, dim3(kThreads), 0, st, grad_out, y, gamma, sample_scale, C, HW, grad_y, part);
  set_last_kernel("convnext_scale_residual_backward");
  if (grad_gamma) launch_reduce(part, B * nblk, C, C, grad_gamma, st);
  return msda::launch_status();
}

size_t patch_embed_hip_layernorm_cf_backward_workspace_bytes(int B, int C, int H, int W) {
  using namespace convnext;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || too_large(B, C, H, W)) return 0;
  return msda::align256((size_t)B * msda::ceil_div(H * W, kLnPx) * 2 * C * sizeof(float));
}

int patch_embed_hip_layernorm_cf_backward_f32(const float* x, const float* weight, float eps, const float* grad_out, int B, int C, int H,
                                              int W, float* grad_x, float* grad_weight, float* grad_bias, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  using namespace convnext;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "layernorm_cf_backward: bad dimensions");
  if (too_large(B, C, H, W)) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "layernorm_cf_backward: problem too large");
  if (!x || !weight || !grad_out) return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "layernorm_cf_backward: null pointer argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (B == 0) {
    if (grad_weight && hipMemsetAsync(grad_weight, 0, (size_t)C * sizeof(float), st) != hipSuccess) return msda::launch_status();
    if (grad_bias && hipMemsetAsync(grad_bias, 0, (size_t)C * sizeof(float), st) != hipSuccess) return msda::launch_status();
    return 0;
  }
  const int HW = H * W, nblk = msda::ceil_div(HW, kLnPx);
  const bool sums = grad_weight || grad_bias;
  if (sums && (!workspace || workspace_bytes < msda::align256((size_t)B * nblk * 2 * C * sizeof(float))))
    return msda::set_error(PATCH_EMBED_ERR_WORKSPACE, "layernorm_cf_backward: workspace too small");
  if (!grad_x && !sums) return 0;
  float* part = sums ? static_cast<float*>(workspace) : nullptr;
  const dim3 grid((unsigned)nblk, (unsigned)B);
  const bool cached = C <= kLnCachedC;
  const int bytes = (int)((2 * kLnThreads + (cached ? (size_t)C * kLnPx : 0)) * sizeof(float));
  if (cached) {
    static std::atomic<uint64_t> done{0};
    const int rc = msda::ensure_dynamic_lds(reinterpret_cast<const void*>(&layernorm_cf_bwd<true>), kLdsBytes, done);
    if (rc) return msda::set_error(rc, "layernorm_cf_backward: cannot reserve LDS");
    hipLaunchKernelGGL((layernorm_cf_bwd<true>), grid, dim3(kLnThreads), bytes, st, x, weight, eps, grad_out, C, HW, grad_x, part);
    set_last_kernel("layernorm_cf_backward<cached>");
  } else {
    hipLaunchKernelGGL((layernorm_cf_bwd<false>), grid, dim3(kLnThreads), bytes, st, x, weight, eps, grad_out, C, HW, grad_x, part);
    set_last_kernel("layernorm_cf_backward<streamed>");
  }
  if (grad_bias) launch_reduce(part, B * nblk, 2 * C, C, grad_bias, st);
  if (grad_weight) launch_reduce(part + C, B * nblk, 2 * C, C, grad_weight, st);
  return msda::launch_status();
}

}  // extern "C"
