// BoxInst training: the box-supervised mask losses and the two target tensors they consume -- see include/dynmask_hip.h
// (criterion_hip_box_bitmasks, criterion_hip_color_similarity_f32, criterion_hip_boxinst_forward_f32 / _backward_f32).
//
//   box bitmasks       one thread per 16 pixels of a row of a box's mask: 16 bytes in one store.  The coordinates are read and
//                      truncated on the device.
//   colour similarity  grid = images x 16 x 16 tiles of the pooled image.  A workgroup pools its tile and a halo of `dilation`
//                      pixels, converts them to Lab in float64 (the sRGB linearisation is a 256-entry table from the host; the cube
//                      root is the only device arithmetic that is not +, *, /) and keeps the fp32 Lab values in LDS; then every pixel
//                      reads its 8 neighbours from there.
//   losses, forward    grid = kept instances x bands of kBand whole rows.  A workgroup forms logsigmoid(+-x) once per pixel of its
//                      band and of `dilation` rows above and below into LDS, adds its pairwise terms in float64, and, owning whole
//                      rows, finds their maxima directly; the columns' maxima of the band go to the workspace.  `boxinst_inst`
//                      (a workgroup per instance) combines the bands' column maxima in band order and forms the instance's dice
//                      sums; `boxinst_finish` (ONE workgroup) adds the instances in a fixed order.
//   losses, backward   grid = rows of src x bands, owner-computes: a pixel adds its 8 terms as a centre and its 8 terms as a
//                      neighbour (those carry the CENTRE's weight), then the projection gradient where it is a recorded maximum.
//
// No float atomics: every sum is the same bits on every call.  Nothing is written that the caller did not lend.
#include "../../include/dynmask_hip.h"

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "wave_ops.hpp"

extern const char* g_criterion_last;   // criterion.hip: what criterion_hip_last_kernel() returns

namespace boxinst {

using msda::f32x4;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBand = 8;                   // rows of a band: 25 bands x 64 instances at the training shape (200 x 336)
constexpr int kTile = 16;                  // the colour similarity's tile: 16 x 16 pooled pixels
constexpr int kMaxDilation = CRITERION_BOXINST_MAX_DILATION;
constexpr int kLdsBytes = 63 * 1024;       // what a workgroup may take without opting in, less the static arrays
constexpr double kDiceEps = 1e-5;          // dice_coefficient (deformable_detr.py:872)

struct Geom {
  int n, N_all, h, w, R, H_im, W_im, stride, start, bands, d, B;
  float thresh;
};

// rows of the LDS tile, and its bytes: two fp32 planes (logsigmoid(x), logsigmoid(-x)) and, for the backward, a byte plane (t)
__host__ __device__ inline int tile_rows(int d) { return kBand + 2 * d; }
inline size_t tile_bytes(int w, int d) { return (size_t)tile_rows(d) * w * 9; }
constexpr int kMaxWidth = kLdsBytes / (9 * (kBand + 2));       // no wider row fits at any dilation

// d l / d x_c of a pairwise term, sigmoid(x_c) - sigmoid(x_c + x_j), without the subtraction (two saturated pixels of one sign
// leave it no digits, and 0 where the true value is 1e-12 of p): with z = x_c + x_j it is -p_c (1 - sigmoid(z)) expm1(x_j), and
// q_c sigmoid(z) expm1(-x_j) is the same number; the branch keeps expm1 away from overflow.  pc, qc = sigmoid(+-x_c).
__device__ __forceinline__ float pair_grad(float pc, float qc, float z, float xj) {
  const float e = expf(-fabsf(z)), r = 1.f / (1.f + e);
  const float m = expm1f(-fabsf(xj));
  return xj < 0.f ? -(pc * (z >= 0.f ? e * r : r)) * m : (qc * (z >= 0.f ? r : e * r)) * m;
}

// The projection term's sigmoid, in float64: with a full target the dice gradient -2 t / U + 4 I p / U^2 cancels to the order of the
// 1e-5 in U, so p, I and U rounded to fp32 would leave it a per cent off.  Only the h + w maxima of an instance pay for it.
__device__ __forceinline__ double sigmoid64(double x) {
  const double e = exp(-fabs(x)), r = 1.0 / (1.0 + e);
  return x >= 0.0 ? r : e * r;
}

// the target byte of pixel (y, x) of an instance whose ground-truth row is `g0` (NULL: out of range, all zero)
__device__ __forceinline__ bool target(const unsigned char* __restrict__ g0, const Geom& g, int y, int x) {
  return g0 && g0[(g.start + (long long)g.stride * y) * g.W_im + g.start + (long long)g.stride * x] != 0;
}

__device__ __forceinline__ const unsigned char* gt_of(const unsigned char* __restrict__ gt, const Geom& g, int r0) {
  return (unsigned)r0 < (unsigned)g.R ? gt + (long long)r0 * g.H_im * g.W_im : nullptr;
}

// Offsets of neighbour k of 8: unfold's order (row-major over the 3 x 3 window) with the centre removed.
__device__ __forceinline__ void offset(int k, int d, int& dy, int& dx) {
  const int c = k < 4 ? k : k + 1;
  dy = (c / 3 - 1) * d;
  dx = (c % 3 - 1) * d;
}

// logsigmoid(+-x) of rows y0 - d .. y0 + kBand + d of one instance into LDS; a row outside the image holds zeros: the unfold's
// padding.  WITH_T also stages the targets.  x_i == NULL reads as logits 0.
template <bool VEC, bool WITH_T>
__device__ __forceinline__ void stage(const float* __restrict__ x_i, const unsigned char* __restrict__ g0, const Geom& g, int y0,
                                      float* __restrict__ lf, float* __restrict__ lb, unsigned char* __restrict__ tp) {
  constexpr int V = VEC ? 4 : 1;
  const int total = tile_rows(g.d) * g.w;
  for (int e = threadIdx.x * V; e < total; e += kThreads * V) {
    const int r = e / g.w, x = e % g.w, y = y0 - g.d + r;
    const bool inside = y >= 0 && y < g.h;
    float v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = 0.f;
    if (inside && x_i) {
      if (VEC) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(x_i + (long long)y * g.w + x);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = q[k];
      } else {
        v[0] = x_i[(long long)y * g.w + x];
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float sp = log1pf(expf(-fabsf(v[k])));
      lf[e + k] = inside ? fminf(v[k], 0.f) - sp : 0.f;
      lb[e + k] = inside ? fminf(-v[k], 0.f) - sp : 0.f;
      if (WITH_T) tp[e + k] = inside && target(g0, g, y, x + k) ? 1 : 0;
    }
  }
}

// ---- the losses: forward -------------------------------------------------------------------------------------------------------
// Workspace of the forward: float64 first, then the 4-byte arrays, then the bytes.  criterion_hip_workspace_bytes is told the
// pixels of an instance, P = h w, not h and w: the arrays are placed for the most bands (P / 8 + 1) and the most band columns
// (bands w <= P / 8 + 7 w / 8 with w <= min(P, kMaxWidth)) that P allows.
struct Work {
  double* part;          // [n, bands, 2]   sum w l, sum w of a band
  double* inst_sums;     // [n, 6]          I_row, U_row, I_col, U_col, sum w l, sum w of an instance
  float* colv;           // [n, bands, w]   the bands' largest logits per column
  int* colp;             // [n, bands, w]   their rows
  unsigned char* colt;   // [n, bands, w]   the bands' largest targets per column
};

inline size_t carve(void* base, long long n, long long P, Work* wk) {
  char* p = static_cast<char*>(base);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* q = p ? p + at : nullptr;
    at += msda::round_up<size_t>(bytes, 16);
    return q;
  };
  const size_t nbw = (size_t)n * (size_t)(P / kBand + std::min<long long>(P, kMaxWidth));
  double* part = reinterpret_cast<double*>(take((size_t)n * (size_t)(P / kBand + 1) * 2 * sizeof(double)));
  double* inst_sums = reinterpret_cast<double*>(take((size_t)n * 6 * sizeof(double)));
  float* colv = reinterpret_cast<float*>(take(nbw * sizeof(float)));
  int* colp = reinterpret_cast<int*>(take(nbw * sizeof(int)));
  unsigned char* colt = reinterpret_cast<unsigned char*>(take(nbw));
  if (wk) *wk = Work{part, inst_sums, colv, colp, colt};
  return at;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads)
boxinst_fwd(const float* __restrict__ src, const int* __restrict__ inst, const unsigned char* __restrict__ gt,
            const int* __restrict__ gt_row, const float* __restrict__ sim, const int* __restrict__ img, Geom g, Work wk,
            int* __restrict__ pos, unsigned char* __restrict__ tmax) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ double red[kWaves][2];
  constexpr int V = VEC ? 4 : 1;
  const int i = blockIdx.x / g.bands, band = blockIdx.x % g.bands;
  const int y0 = band * kBand, rows = min(kBand, g.h - y0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* lf = reinterpret_cast<float*>(lds);
  float* lb = lf + tile_rows(g.d) * g.w;
  const int r = inst[i];
  const float* __restrict__ x_i = (unsigned)r < (unsigned)g.N_all ? src + (long long)r * g.h * g.w : nullptr;
  const unsigned char* __restrict__ g0 = gt_of(gt, g, gt_row[i]);
  const int b = img[i];
  const float* __restrict__ sim_i = (unsigned)b < (unsigned)g.B ? sim + (long long)b * 8 * g.h * g.w : nullptr;
  stage<VEC, false>(x_i, g0, g, y0, lf, lb, nullptr);
  __syncthreads();

  // the pairwise term: l = -LSE(lf_i + lf_j, lb_i + lb_j), weight (sim >= thresh) t_i
  double acc[2] = {0.0, 0.0};
  const long long plane = (long long)g.h * g.w;
  for (int e = threadIdx.x * V; e < rows * g.w && sim_i; e += kThreads * V) {
    const int ly = e / g.w, x = e % g.w, y = y0 + ly;
    bool t[V], any = false;
#pragma unroll
    for (int k = 0; k < V; ++k) any |= t[k] = target(g0, g, y, x + k);
    if (!any) continue;
    const int c = (ly + g.d) * g.w + x;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int dy, dx;
      offset(k, g.d, dy, dx);
      float s[V];
      const float* __restrict__ sp = sim_i + k * plane + (long long)y * g.w + x;
      if (VEC) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(sp);
#pragma unroll
        for (int v = 0; v < V; ++v) s[v] = q[v];
      } else {
        s[0] = sp[0];
      }
      const bool row_in = y + dy >= 0 && y + dy < g.h;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (!(t[v] && s[v] >= g.thresh)) continue;
        const int xn = x + v + dx;
        const bool in = row_in && xn >= 0 && xn < g.w;
        const int j = c + v + dy * g.w + dx;
        const float a = lf[c + v] + (in ? lf[j] : 0.f), bb = lb[c + v] + (in ? lb[j] : 0.f);
        const float lse = fmaxf(a, bb) + log1pf(expf(-fabsf(a - bb)));
        acc[0] -= (double)lse;
        acc[1] += 1.0;
      }
    }
  }
  wave_ops::block_sum<2, kWaves>(acc, red);
  if (threadIdx.x == 0) {
    wk.part[(long long)blockIdx.x * 2] = acc[0];
    wk.part[(long long)blockIdx.x * 2 + 1] = acc[1];
  }

  // the rows of the band: a wave per row; the largest logit, the lowest column among equals
  for (int ly = wv; ly < rows; ly += kWaves) {
    const int y = y0 + ly;
    float best = -INFINITY;
    int at = INT_MAX, tm = 0;
    for (int x = lane; x < g.w; x += 64) {
      const float v = x_i ? x_i[(long long)y * g.w + x] : 0.f;
      if (v > best || at == INT_MAX) { best = v; at = x; }
      tm |= target(g0, g, y, x) ? 1 : 0;
    }
    wave_ops::wave_argmax(best, at);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tm |= __shfl_xor(tm, o, 64);
    if (lane == 0) {
      pos[(long long)i * (g.h + g.w) + y] = at;
      tmax[(long long)i * (g.h + g.w) + y] = (unsigned char)tm;
    }
  }
  // the columns of the band: a thread per column; the lowest row among equals
  for (int x = threadIdx.x; x < g.w; x += kThreads) {
    float best = x_i ? x_i[(long long)y0 * g.w + x] : 0.f;
    int at = y0, tm = target(g0, g, y0, x) ? 1 : 0;
    for (int ly = 1; ly < rows; ++ly) {
      const float v = x_i ? x_i[(long long)(y0 + ly) * g.w + x] : 0.f;
      if (v > best) { best = v; at = y0 + ly; }
      tm |= target(g0, g, y0 + ly, x) ? 1 : 0;
    }
    const long long o = (long long)blockIdx.x * g.w + x;
    wk.colv[o] = best;
    wk.colp[o] = at;
    wk.colt[o] = (unsigned char)tm;
  }
}

// One workgroup per instance: the bands' column maxima combined in band order (lowest row among equals), the dice sums of the rows
// and of the columns, the bands' pairwise sums in band order.  sums [n, 4] (float64) = I_row, U_row, I_col, U_col for the backward.
__global__ void __launch_bounds__(kThreads)
boxinst_inst(const float* __restrict__ src, const int* __restrict__ inst, Geom g, Work wk, int* __restrict__ pos,
             unsigned char* __restrict__ tmax, double* __restrict__ sums) {
  __shared__ double red[kWaves][6];
  const int i = blockIdx.x;
  const int r = inst[i];
  const float* __restrict__ x_i = (unsigned)r < (unsigned)g.N_all ? src + (long long)r * g.h * g.w : nullptr;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int y = threadIdx.x; y < g.h; y += kThreads) {
    const int at = pos[(long long)i * (g.h + g.w) + y];
    const double p = sigmoid64(x_i ? (double)x_i[(long long)y * g.w + at] : 0.0), t = (double)tmax[(long long)i * (g.h + g.w) + y];
    acc[0] += p * t;
    acc[1] += p * p + t * t;
  }
  for (int x = threadIdx.x; x < g.w; x += kThreads) {
    long long o = (long long)i * g.bands * g.w + x;
    float best = wk.colv[o];
    int at = wk.colp[o], tm = wk.colt[o];
    for (int b = 1; b < g.bands; ++b) {
      o += g.w;
      const float v = wk.colv[o];
      if (v > best) { best = v; at = wk.colp[o]; }
      tm |= wk.colt[o];
    }
    pos[(long long)i * (g.h + g.w) + g.h + x] = at;
    tmax[(long long)i * (g.h + g.w) + g.h + x] = (unsigned char)tm;
    const double p = sigmoid64((double)best), t = (double)tm;
    acc[2] += p * t;
    acc[3] += p * p + t * t;
  }
  for (int b = threadIdx.x; b < g.bands; b += kThreads) {
    acc[4] += wk.part[((long long)i * g.bands + b) * 2];
    acc[5] += wk.part[((long long)i * g.bands + b) * 2 + 1];
  }
  wave_ops::block_sum<6, kWaves>(acc, red);
  if (threadIdx.x == 0) {
    acc[1] += kDiceEps;
    acc[3] += kDiceEps;
#pragma unroll
    for (int k = 0; k < 6; ++k) wk.inst_sums[(long long)i * 6 + k] = acc[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) sums[(long long)i * 4 + k] = acc[k];
  }
}

// losses = (mean_i (dice_col + dice_row), warmup * sum w l / max(sum w, 1)); totals = (sum w l, sum w)
__global__ void __launch_bounds__(kThreads)
boxinst_finish(const double* __restrict__ inst_sums, int n, const float* __restrict__ warmup, float* __restrict__ losses,
               double* __restrict__ totals) {
  __shared__ double red[kWaves][3];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const double* s = inst_sums + (long long)i * 6;
    acc[0] += (1.0 - 2.0 * s[0] / s[1]) + (1.0 - 2.0 * s[2] / s[3]);
    acc[1] += s[4];
    acc[2] += s[5];
  }
  wave_ops::block_sum<3, kWaves>(acc, red);
  if (threadIdx.x == 0) {
    losses[0] = (float)(acc[0] / (double)n);
    losses[1] = (float)((double)warmup[0] * (acc[1] / fmax(acc[2], 1.0)));
    totals[0] = acc[1];
    totals[1] = acc[2];
  }
}

// ---- the losses: backward ------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
boxinst_bwd(const float* __restrict__ src, const int* __restrict__ inst, const unsigned char* __restrict__ gt,
            const int* __restrict__ gt_row, const float* __restrict__ sim, const int* __restrict__ img, Geom g,
            const int* __restrict__ pos, const unsigned char* __restrict__ tmax, const double* __restrict__ sums,
            const double* __restrict__ totals, const float* __restrict__ warmup, const float* __restrict__ g_prj_ptr,
            const float* __restrict__ g_pair_ptr, float* __restrict__ grad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int owner;
  constexpr int V = VEC ? 4 : 1;
  const int r = blockIdx.x / g.bands, band = blockIdx.x % g.bands;
  const int y0 = band * kBand, rows = min(kBand, g.h - y0);
  float* __restrict__ out = grad + (long long)r * g.h * g.w + (long long)y0 * g.w;
  if (threadIdx.x == 0) owner = INT_MAX;
  __syncthreads();
  for (int k = threadIdx.x; k < g.n; k += kThreads)
    if (inst[k] == r) atomicMin(&owner, k);          // LDS; the rows of `inst` are distinct, the lowest wins if they are not
  __syncthreads();
  const int i = owner;
  if (i == INT_MAX) {                                // a row no kept instance reads: exactly 0.0
    for (int e = threadIdx.x * V; e < rows * g.w; e += kThreads * V) {
      if (VEC) *reinterpret_cast<f32x4*>(out + e) = f32x4{0.f, 0.f, 0.f, 0.f};
      else out[e] = 0.f;
    }
    return;
  }
  const int tr = tile_rows(g.d);
  float* lf = reinterpret_cast<float*>(lds);
  float* lb = lf + tr * g.w;
  unsigned char* tp = reinterpret_cast<unsigned char*>(lb + tr * g.w);
  const float* __restrict__ x_i = src + (long long)r * g.h * g.w;
  const unsigned char* __restrict__ g0 = gt_of(gt, g, gt_row[i]);
  const int b = img[i];
  const float* __restrict__ sim_i = (unsigned)b < (unsigned)g.B ? sim + (long long)b * 8 * g.h * g.w : nullptr;
  stage<VEC, true>(x_i, g0, g, y0, lf, lb, tp);
  __syncthreads();

  const float scale = (float)((double)g_pair_ptr[0] * (double)warmup[0] / fmax(totals[1], 1.0));
  const double cprj = (double)g_prj_ptr[0] / (double)g.n;
  const double I_r = sums[4 * i], U_r = sums[4 * i + 1], I_c = sums[4 * i + 2], U_c = sums[4 * i + 3];
  const int* __restrict__ pos_i = pos + (long long)i * (g.h + g.w);
  const unsigned char* __restrict__ tm_i = tmax + (long long)i * (g.h + g.w);
  const long long plane = (long long)g.h * g.w;
  for (int e = threadIdx.x * V; e < rows * g.w; e += kThreads * V) {
    const int ly = e / g.w, x = e % g.w, y = y0 + ly;
    const int c = (ly + g.d) * g.w + x;
    float res[V];
#pragma unroll
    for (int v = 0; v < V; ++v) res[v] = 0.f;
    if (sim_i) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        int dy, dx;
        offset(k, g.d, dy, dx);
        // as a centre: the neighbour at (y + dy, x + dx); outside the image its log-probabilities are 0 and the term's gradient too
        const bool down = y + dy >= 0 && y + dy < g.h;
        // as a neighbour: the centre at (y - dy, x - dx) carries the weight and the similarity
        const bool up = y - dy >= 0 && y - dy < g.h;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const int xv = x + v, cv = c + v;
          const float p = expf(lf[cv]), q = expf(lb[cv]);
          const int xn = xv + dx, xc = xv - dx;
          if (down && xn >= 0 && xn < g.w && tp[cv] && sim_i[k * plane + (long long)y * g.w + xv] >= g.thresh) {
            const int j = cv + dy * g.w + dx;
            res[v] += pair_grad(p, q, (lf[cv] + lf[j]) - (lb[cv] + lb[j]), lf[j] - lb[j]);
          }
          if (up && xc >= 0 && xc < g.w) {
            const int j = cv - dy * g.w - dx;
            if (tp[j] && sim_i[k * plane + (long long)(y - dy) * g.w + xc] >= g.thresh)
              res[v] += pair_grad(p, q, (lf[j] + lf[cv]) - (lb[j] + lb[cv]), lf[j] - lb[j]);
          }
        }
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int xv = x + v;
      res[v] *= scale;
      const bool row_max = pos_i[y] == xv, col_max = pos_i[g.h + xv] == y;
      if (row_max || col_max) {                      // the projection gradient, in float64 (sigmoid64)
        const double p = sigmoid64((double)x_i[(long long)y * g.w + xv]), q = sigmoid64(-(double)x_i[(long long)y * g.w + xv]);
        double gp = 0.0;
        if (row_max) gp += (4.0 * I_r * p - 2.0 * (double)tm_i[y] * U_r) / (U_r * U_r);
        if (col_max) gp += (4.0 * I_c * p - 2.0 * (double)tm_i[g.h + xv] * U_c) / (U_c * U_c);
        res[v] += (float)(cprj * gp * (p * q));
      }
    }
    if (VEC) *reinterpret_cast<f32x4*>(out + e) = f32x4{res[0], res[V > 1 ? 1 : 0], res[V > 2 ? 2 : 0], res[V > 3 ? 3 : 0]};
    else out[e] = res[0];
  }
}

// ---- box bitmasks --------------------------------------------------------------------------------------------------------------
typedef unsigned int u32x4 __attribute__((__vector_size__(16)));

// [int(y1) : int(y2 + 1), int(x1) : int(x2 + 1)] as a slice takes it: truncation toward zero, the far ends clamped
__device__ __forceinline__ int trunc_clamped(float v, int most) {
  return v >= (float)most ? most : (v > -1.f ? (int)v : (v != v ? most : 0));
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads)
box_bitmasks(const float* __restrict__ boxes, int G, int H, int W, unsigned char* __restrict__ out) {
  constexpr int V = VEC ? 16 : 1;
  const long long per_row = W / V, total = (long long)G * H * per_row;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
    const int xg = (int)(e % per_row) * V;
    const long long gy = e / per_row;
    const int y = (int)(gy % H), b = (int)(gy / H);
    const float* __restrict__ box = boxes + 4 * (long long)b;
    const int x_lo = trunc_clamped(box[0], W), x_hi = trunc_clamped(box[2] + 1.f, W);
    const int y_lo = trunc_clamped(box[1], H), y_hi = trunc_clamped(box[3] + 1.f, H);
    const bool row = y >= y_lo && y < y_hi;
    if (VEC) {
      u32x4 q = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (row && xg + k >= x_lo && xg + k < x_hi) q[k / 4] |= 1u << (8 * (k % 4));
      *reinterpret_cast<u32x4*>(out + gy * W + xg) = q;
    } else {
      out[gy * W + xg] = row && xg >= x_lo && xg < x_hi ? 1 : 0;
    }
  }
}

// ---- colour similarity ---------------------------------------------------------------------------------------------------------
struct SimGeom {
  int bs, H, W, h, w, stride, start, d, tiles_x, tiles_y, kind;
};

// skimage.color.rgb2lab of one pixel whose channels went through the linearisation table: D65, observer 2
__device__ __forceinline__ void lab_of(double r, double gch, double b, float (&lab)[3]) {
  double xyz[3] = {0.412453 * r + 0.357580 * gch + 0.180423 * b, 0.212671 * r + 0.715160 * gch + 0.072169 * b,
                   0.019334 * r + 0.119193 * gch + 0.950227 * b};
  const double white[3] = {0.95047, 1.0, 1.08883};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double t = xyz[k] / white[k];
    xyz[k] = t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0;
  }
  lab[0] = (float)(116.0 * xyz[1] - 16.0);
  lab[1] = (float)(500.0 * (xyz[0] - xyz[1]));
  lab[2] = (float)(200.0 * (xyz[1] - xyz[2]));
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
color_similarity(const T* __restrict__ images, const unsigned char* __restrict__ mask, const double* __restrict__ table, SimGeom g,
                 float* __restrict__ out, float* __restrict__ lab_out) {
  __shared__ float tile[3][kTile + 2 * kMaxDilation][kTile + 2 * kMaxDilation + 1];
  const int per = g.tiles_x * g.tiles_y;
  const int b = blockIdx.x / per, ty = blockIdx.x % per / g.tiles_x, tx = blockIdx.x % g.tiles_x;
  const int y0 = ty * kTile - g.d, x0 = tx * kTile - g.d, side = kTile + 2 * g.d;
  const long long plane = (long long)g.H * g.W;
  const T* __restrict__ im = images + (long long)b * 3 * plane;
  for (int e = threadIdx.x; e < side * side; e += kThreads) {
    const int ly = e / side, lx = e % side, y = y0 + ly, x = x0 + lx;
    float lab[3] = {0.f, 0.f, 0.f};
    if (y >= 0 && y < g.h && x >= 0 && x < g.w) {
      double lin[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {                 // avg_pool2d in fp32, .byte(): truncation
        float s = 0.f;
        for (int dy = 0; dy < g.stride; ++dy)
          for (int dx = 0; dx < g.stride; ++dx)
            s += (float)im[ch * plane + (long long)(y * g.stride + dy) * g.W + x * g.stride + dx];
        const int byte = (int)fminf(fmaxf(s / (float)(g.stride * g.stride), 0.f), 255.f);
        lin[ch] = table[byte];
      }
      lab_of(lin[2], lin[1], lin[0], lab);             // the images are BGR
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) tile[ch][ly][lx] = lab[ch];
  }
  __syncthreads();
  const int ly = threadIdx.x / kTile, lx = threadIdx.x % kTile;
  const int y = ty * kTile + ly, x = tx * kTile + lx;
  if (y >= g.h || x >= g.w) return;
  const int cy = ly + g.d, cx = lx + g.d;
  const long long small = (long long)g.h * g.w, at = (long long)y * g.w + x;
  if (lab_out) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) lab_out[((long long)b * 3 + ch) * small + at] = tile[ch][cy][cx];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int dy, dx;
    offset(k, g.d, dy, dx);
    const int yn = y + dy, xn = x + dx;
    float v = 0.f;
    if (yn >= 0 && yn < g.h && xn >= 0 && xn < g.w &&
        mask[(long long)b * plane + (long long)(g.start + g.stride * yn) * g.W + g.start + g.stride * xn]) {
      const float a0 = tile[0][cy][cx] - tile[0][cy + dy][cx + dx], a1 = tile[1][cy][cx] - tile[1][cy + dy][cx + dx],
                  a2 = tile[2][cy][cx] - tile[2][cy + dy][cx + dx];
      v = expf(-sqrtf(a0 * a0 + a1 * a1 + a2 * a2) * 0.5f);
    }
    out[((long long)b * 8 + k) * small + at] = v;
  }
}

}  // namespace boxinst

// CRITERION_BOXINST of criterion_hip_workspace_bytes (criterion.hip): n instances of P = h w pixels
size_t boxinst_workspace_bytes(long long n, long long P) { return boxinst::carve(nullptr, n, P, nullptr); }

extern "C" {

int criterion_hip_box_bitmasks(const float* boxes, int G, int H, int W, unsigned char* out, void* stream) {
  if (G < 0 || H <= 0 || W <= 0) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_box_bitmasks: bad dimensions");
  if ((long long)G * H * W >= (1ll << 40)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_box_bitmasks: problem too large");
  if (G == 0) return 0;
  if (!boxes || !out) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_box_bitmasks: null pointer argument");
  const bool vec = W % 16 == 0 && msda::aligned16({out});
  const long long work = (long long)G * H * (vec ? W / 16 : W);
  const long long blocks = std::min<long long>(msda::ceil_div<long long>(work, boxinst::kThreads), 2048);
  auto kernel = vec ? boxinst::box_bitmasks<true> : boxinst::box_bitmasks<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(boxinst::kThreads), 0, (hipStream_t)stream, boxes, G, H, W, out);
  if (const int rc = msda::launch_status()) return rc;
  g_criterion_last = vec ? "box_bitmasks<vec4>" : "box_bitmasks<scalar>";
  return 0;
}

int criterion_hip_color_similarity_f32(const void* images, int image_kind, const unsigned char* mask, const double* table, int bs,
                                       int H, int W, int stride, int dilation, float* out, float* lab, void* stream) {
  if (bs < 0 || H <= 0 || W <= 0 || stride <= 0 || H % stride || W % stride)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_color_similarity: bad dimensions");
  if (dilation < 1 || dilation > boxinst::kMaxDilation)
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "criterion_color_similarity: dilation outside 1 .. 8");
  if (image_kind != CRITERION_IMAGE_U8 && image_kind != CRITERION_IMAGE_F32)
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "criterion_color_similarity: unknown image kind");
  if ((long long)bs * 3 * H * W >= (1ll << 40)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_color_similarity: problem too large");
  if (bs == 0) return 0;
  if (!images || !mask || !table || !out) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_color_similarity: null pointer argument");
  const int h = H / stride, w = W / stride;
  const int tiles_x = msda::ceil_div(w, boxinst::kTile), tiles_y = msda::ceil_div(h, boxinst::kTile);
  if ((long long)bs * tiles_x * tiles_y >= (1ll << 31)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_color_similarity: problem too large");
  const boxinst::SimGeom g{bs, H, W, h, w, stride, stride / 2, dilation, tiles_x, tiles_y, image_kind};
  const dim3 grid((unsigned)(bs * tiles_x * tiles_y));
  if (image_kind == CRITERION_IMAGE_U8)
    hipLaunchKernelGGL(boxinst::color_similarity<unsigned char>, grid, dim3(boxinst::kThreads), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(images), mask, table, g, out, lab);
  else
    hipLaunchKernelGGL(boxinst::color_similarity<float>, grid, dim3(boxinst::kThreads), 0, (hipStream_t)stream,
                       static_cast<const float*>(images), mask, table, g, out, lab);
  if (const int rc = msda::launch_status()) return rc;
  g_criterion_last = image_kind == CRITERION_IMAGE_U8 ? "color_similarity<u8>" : "color_similarity<f32>";
  return 0;
}

// 0 with `g` filled, 1 for an empty problem, or an error code
static int boxinst_args(const char* who, const float* src, const int32_t* inst, const unsigned char* gt, const int32_t* gt_row,
                        const float* sim, const int32_t* img, int n, int N_all, int F, int h, int w, int R, int H_im, int W_im,
                        int stride, int B, float thresh, int dilation, boxinst::Geom* g) {
  if (n < 0 || N_all < 0 || F <= 0 || h <= 0 || w <= 0 || R < 0 || H_im <= 0 || W_im <= 0 || stride <= 0 || B < 0)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, who);
  if (F != 1) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "criterion_boxinst: one frame an instance (frames != 1)");
  if (dilation < 1 || dilation > boxinst::kMaxDilation)
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "criterion_boxinst: dilation outside 1 .. 8");
  if (boxinst::tile_bytes(w, dilation) > (size_t)boxinst::kLdsBytes)
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "criterion_boxinst: rows too wide for the LDS tile");
  const int start = stride / 2;
  if (start + (long long)stride * (h - 1) >= H_im || start + (long long)stride * (w - 1) >= W_im)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_boxinst: the strided pixels do not fit the ground-truth masks");
  const int bands = msda::ceil_div(h, boxinst::kBand);
  const long long P = (long long)h * w;
  if (P >= (1ll << 28) || (long long)N_all * P >= (1ll << 40) || (long long)R * H_im * W_im >= (1ll << 40) ||
      (long long)B * 8 * P >= (1ll << 40) || (long long)std::max(n, N_all) * bands >= (1ll << 31))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "criterion_boxinst: problem too large");
  *g = boxinst::Geom{n, N_all, h, w, R, H_im, W_im, stride, start, bands, dilation, B, thresh};
  if (n == 0) return 1;
  if (!src || !inst || !gt || !gt_row || !sim || !img) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_boxinst: null pointer argument");
  return 0;
}

int criterion_hip_boxinst_forward_f32(const float* src, const int32_t* inst, const unsigned char* gt, const int32_t* gt_row,
                                      const float* sim, const int32_t* img, const float* warmup, int n, int N_all, int F, int h, int w,
                                      int R, int H_im, int W_im, int stride, int B, float thresh, int dilation, int32_t* pos,
                                      unsigned char* tmax, double* sums, double* totals, float* losses, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  boxinst::Geom g;
  const int e = boxinst_args("criterion_boxinst_forward: bad dimensions", src, inst, gt, gt_row, sim, img, n, N_all, F, h, w, R, H_im,
                             W_im, stride, B, thresh, dilation, &g);
  if (e < 0 || e > 1) return e;
  if (!losses || !totals) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_boxinst_forward: null pointer argument");
  if (e == 1) {
    if (const int rc = msda::launch_status((int)hipMemsetAsync(losses, 0, 2 * sizeof(float), (hipStream_t)stream))) return rc;
    return msda::launch_status((int)hipMemsetAsync(totals, 0, 2 * sizeof(double), (hipStream_t)stream));
  }
  if (!warmup || !pos || !tmax || !sums) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_boxinst_forward: null pointer argument");
  if (!workspace || workspace_bytes < boxinst_workspace_bytes(n, (long long)h * w) || !msda::aligned16({workspace}))
    return msda::set_error(CRITERION_ERR_WORKSPACE, "criterion_boxinst_forward: workspace too small or not 16-byte aligned");
  boxinst::Work wk;
  boxinst::carve(workspace, n, (long long)h * w, &wk);
  const bool vec = w % 4 == 0 && msda::aligned16({src, sim});
  const size_t lds = boxinst::tile_bytes(w, dilation);
  auto kernel = vec ? boxinst::boxinst_fwd<true> : boxinst::boxinst_fwd<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(n * g.bands)), dim3(boxinst::kThreads), lds, (hipStream_t)stream, src, inst, gt, gt_row,
                     sim, img, g, wk, pos, tmax);
  hipLaunchKernelGGL(boxinst::boxinst_inst, dim3((unsigned)n), dim3(boxinst::kThreads), 0, (hipStream_t)stream, src, inst, g, wk, pos, tmax,
                     sums);
  hipLaunchKernelGGL(boxinst::boxinst_finish, dim3(1), dim3(boxinst::kThreads), 0, (hipStream_t)stream, wk.inst_sums, n, warmup, losses,
                     totals);
  if (const int rc = msda::launch_status()) return rc;
  g_criterion_last = vec ? "boxinst_fwd<vec4>" : "boxinst_fwd<scalar>";
  return 0;
}

int criterion_hip_boxinst_backward_f32(const float* src, const int32_t* inst, const unsigned char* gt, const int32_t* gt_row,
                                       const float* sim, const int32_t* img, const float* warmup, const int32_t* pos,
                                       const unsigned char* tmax, const double* sums, const double* totals, const float* grad_prj,
                                       const float* grad_pairwise, int n, int N_all, int F, int h, int w, int R, int H_im, int W_im,
                                       int stride, int B, float thresh, int dilation, float* grad_src, void* stream) {
  boxinst::Geom g;
  const int e = boxinst_args("criterion_boxinst_backward: bad dimensions", src, inst, gt, gt_row, sim, img, n, N_all, F, h, w, R, H_im,
                             W_im, stride, B, thresh, dilation, &g);
  if (e < 0 || e > 1) return e;
  if (N_all == 0) return 0;
  if (!grad_src) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_boxinst_backward: null pointer argument");
  if (e == 1)
    return msda::launch_status((int)hipMemsetAsync(grad_src, 0, (size_t)N_all * h * w * sizeof(float), (hipStream_t)stream));
  if (!warmup || !pos || !tmax || !sums || !totals || !grad_prj || !grad_pairwise)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "criterion_boxinst_backward: null pointer argument");
  const bool vec = w % 4 == 0 && msda::aligned16({src, sim, grad_src});
  const size_t lds = boxinst::tile_bytes(w, dilation);
  auto kernel = vec ? boxinst::boxinst_bwd<true> : boxinst::boxinst_bwd<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(N_all * g.bands)), dim3(boxinst::kThreads), lds, (hipStream_t)stream, src, inst, gt, gt_row,
                     sim, img, g, pos, tmax, sums, totals, warmup, grad_prj, grad_pairwise, grad_src);
  if (const int rc = msda::launch_status()) return rc;
  g_criterion_last = vec ? "boxinst_bwd<vec4>" : "boxinst_bwd<scalar>";
  return 0;
}

}  // extern "C"
