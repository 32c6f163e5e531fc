// Backward of the patch-embedding convolutions (kernel == stride, no padding) of patch_embed.hip -- see
// include/patch_embed_hip.h.  With the forward's notation (m = (b, py, px) patch, e = output channel, kk = (c, ky, kx)):
//
//   A[m, kk] = x[b, c, py*KS + ky, px*KS + kx]                 G[m, e] = grad_out   ([B, Hp, Wp, E] or [B, E, Hp, Wp])
//   grad_weight[e, kk] = sum_m G[m, e] * A[m, kk]          grad_bias[e] = sum_m G[m, e]
//   grad_x[b, c, py*KS + ky, px*KS + kx] = sum_e G[m, e] * W[e, kk]       (0 in the rows / columns past Hp*KS, Wp*KS)
//
// Both products are the forward's GEMM with other operands: 2 x 2 waves, v_mfma_f32_32x32x2_f32, operand tiles staged
// through double-buffered LDS as [row][16 reduction indices] (80-byte pitch), one ds_read_b128 per half-wave feeding four
// MFMAs.  Exact fp32 products, fp32 accumulation in a fixed order, no float atomics: bitwise repeatable.
//   * patch_wgrad: rows = e, columns = kk, reduction over m in 16-patch chunks.  A is read in place from x with the forward's
//     addressing (lanes along the kx runs of consecutive patches); the m range is split into a number of ranges that depends
//     on the shape only, each workgroup writes its partial tile to the workspace and wgrad_reduce adds the slabs in split
//     order (with one split the tile goes straight to grad_weight).  The workgroups of the first kk tile also sum the G
//     values they stage into per-split bias partials.
//   * patch_colsum: grad_bias alone -- the same per-split partial sums without the GEMM.
//   * patch_dgrad: rows = kk, columns = m (the transposed accumulator puts lanes along consecutive patches, so for a fixed
//     (c, ky) the stores of a kx run coalesce like the forward's loads), reduction over e.  zero_remainder writes the zeros
//     of the pixels no patch covers, and only those.
#include "../../include/patch_embed_hip.h"

#include "gemm_core.hpp"
#include "launch_glue.hpp"

namespace patch_embed_bwd {

constexpr int kThreads = 256;
constexpr int BR = 16;                     // reduction indices per LDS stage
constexpr int kPitch = 20;                 // floats per LDS row: 16 + 4 pad (rows stay 16-byte aligned)
constexpr int kTargetGroups = 512;         // grad-weight workgroups a launch aims at (2 per CU of the MI355X)
constexpr int kMaxSplits = 256;
constexpr int kMinChunksPerSplit = 8;      // at least 128 patches per split

using namespace gemm_core;
using msda::align256;

struct Geom {
  int B, C, H, W, E, Hp, Wp, M, K;
};

// grad-weight tile: 64 x 64 when the GEMM is short in either direction (ConvNeXt stem: E x K = 192 x 48), else 128 x 128
inline bool wgrad_small(int E, int K) { return K <= 64 || E <= 64; }

inline int wgrad_splits(long long M, int E, int K) {
  const int t = wgrad_small(E, K) ? 64 : 128;
  const long long tiles = (long long)((E + t - 1) / t) * ((K + t - 1) / t);
  const long long chunks = (M + BR - 1) / BR;
  long long s = (kTargetGroups + tiles - 1) / tiles;
  if (s > kMaxSplits) s = kMaxSplits;
  if (s > chunks / kMinChunksPerSplit) s = chunks / kMinChunksPerSplit;
  return s < 1 ? 1 : (int)s;
}

struct Layout {   // byte offsets of the workspace parts
  size_t wparts, bparts, total;
  int splits;
};

inline Layout layout(long long M, int E, int K) {
  Layout l;
  l.splits = wgrad_splits(M, E, K);
  l.wparts = 0;
  if (l.splits == 1) {   // the kernels write the gradients themselves; the minimum keeps the query's 0 for "unsupported"
    l.bparts = 0;
    l.total = 256;
    return l;
  }
  l.bparts = align256((size_t)l.splits * E * K * sizeof(float));
  l.total = l.bparts + align256((size_t)l.splits * E * sizeof(float));
  return l;
}

// offset of x[b, 0, py*KS, px*KS] for patch m
template <int KS>
__device__ __forceinline__ int64_t patch_base(int m, const Geom& g) {
  const int HpWp = g.Hp * g.Wp;
  const int b = m / HpWp, sp = m - b * HpWp;
  const int py = sp / g.Wp, px = sp - py * g.Wp;
  return ((int64_t)b * g.C * g.H + (int64_t)py * KS) * g.W + (int64_t)px * KS;
}

// ------------------------------------------------------------------------------------------------
// grid (e tiles x kk tiles, splits).  Gs[e][16 m], As[kk][16 m]; out = this split's slab [E][K] (grad_weight itself with one
// split), bparts = this split's bias partials [E] (nullptr: no bias; only the first kk tile writes them).
template <int KS, bool NHWC, int BE, int BKK>
__global__ void __launch_bounds__(kThreads, 2)
patch_wgrad(const float* __restrict__ x, const float* __restrict__ gout, Geom g, int splits, float* __restrict__ wout,
            float* __restrict__ bout) {
  constexpr int VW = KS >= 4 ? 4 : 2;                  // floats per A load (a kx run piece)
  constexpr int PP = KS / VW;                          // pieces per kx run
  constexpr int kALoads = BKK * BR / VW / kThreads;    // A items per thread and stage
  constexpr int kGLoads = BE * BR / 4 / kThreads;      // G items (4 values) per thread and stage
  static_assert(kALoads >= 1 && kGLoads >= 1, "tile");
  constexpr int TI = BE / 64, TJ = BKK / 64;
  __shared__ __attribute__((aligned(16))) float Gs[2][BE][kPitch];
  __shared__ __attribute__((aligned(16))) float As[2][BKK][kPitch];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ntk = (g.K + BKK - 1) / BKK;
  const int e0 = (blockIdx.x / ntk) * BE, kk0 = (blockIdx.x % ntk) * BKK;
  const int split = blockIdx.y;
  const long long chunks = ((long long)g.M + BR - 1) / BR;
  const int c_begin = (int)(chunks * split / splits), c_end = (int)(chunks * (split + 1) / splits);
  const int m_end = c_end * BR < g.M ? c_end * BR : g.M;
  const bool do_bias = bout != nullptr && kk0 == 0;
  const int HpWp = g.Hp * g.Wp;

  // ---- A items: piece i % PP of the kx run of (patch row (i / PP) % 16, run i / (16 PP)); the patch row is the same for
  // all of a thread's items, so one patch decode per stage serves them all
  const int a_mrow = (tid / PP) % BR;
  int64_t a_off[kALoads];
  int a_kk[kALoads];
  bool a_ok[kALoads];
#pragma unroll
  for (int r = 0; r < kALoads; ++r) {
    const int i = tid + r * kThreads;
    const int kk = kk0 + (i / (PP * BR)) * KS + (i % PP) * VW;
    a_kk[r] = kk - kk0;
    a_ok[r] = kk < g.K;
    const int kc = a_ok[r] ? kk : 0;
    const int c = kc / (KS * KS), rr = kc % (KS * KS);
    a_off[r] = ((int64_t)c * g.H + rr / KS) * g.W + rr % KS;
  }
  // ---- G items.  NHWC: 4 consecutive e (group i / 16) of patch row i % 16 -- the lanes run along the patches, so the
  //      transposed LDS stores of a wave hit 64 different banks.  NCHW: 4 consecutive patches (quad i % 4) of channel row i / 4.
  //      Either way a thread's patch row / quad is the same for all its items: its bias sums are per (item, value).
  float bsum[kGLoads][4] = {};

  float a_reg[kALoads][VW];
  float g_reg[kGLoads][4];
  auto load_stage = [&](int ch) {
    const int m0 = ch * BR;
    {
      const int m = m0 + a_mrow;
      const bool ok = m < m_end;
      const int64_t base = patch_base<KS>(ok ? m : 0, g);
#pragma unroll
      for (int r = 0; r < kALoads; ++r) {
        const float* p = x + base + a_off[r];
        const bool v = ok && a_ok[r];
#pragma unroll
        for (int e = 0; e < VW; ++e) a_reg[r][e] = v ? p[e] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < kGLoads; ++r) {
      const int i = tid + r * kThreads;
      if constexpr (NHWC) {
        const int mrow = i % BR, eg = i / BR;
        const int m = m0 + mrow, e = e0 + eg * 4;
        const float* p = gout + (int64_t)m * g.E + e;
        if (m < m_end && e + 3 < g.E) {
#pragma unroll
          for (int q = 0; q < 4; ++q) g_reg[r][q] = p[q];
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) g_reg[r][q] = (m < m_end && e + q < g.E) ? p[q] : 0.f;
        }
      } else {
        const int mq = i % 4, erow = i / 4;
        const int e = e0 + erow;
        int m = m0 + mq * 4;
        int b = m / HpWp, sp = m - b * HpWp;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          g_reg[r][q] = (m < m_end && e < g.E) ? gout[((int64_t)b * g.E + e) * HpWp + sp] : 0.f;
          ++m;
          if (++sp == HpWp) { sp = 0; ++b; }
        }
      }
    }
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int r = 0; r < kALoads; ++r)
#pragma unroll
      for (int e = 0; e < VW; ++e) As[buf][a_kk[r] + e][a_mrow] = a_reg[r][e];
#pragma unroll
    for (int r = 0; r < kGLoads; ++r) {
      const int i = tid + r * kThreads;
      if constexpr (NHWC) {
        const int mrow = i % BR, eg = i / BR;
#pragma unroll
        for (int q = 0; q < 4; ++q) Gs[buf][eg * 4 + q][mrow] = g_reg[r][q];
        if (do_bias) {
#pragma unroll
          for (int q = 0; q < 4; ++q) bsum[r][q] += g_reg[r][q];
        }
      } else {
        const int mq = i % 4, erow = i / 4;
        *reinterpret_cast<f32x4*>(&Gs[buf][erow][mq * 4]) = f32x4{g_reg[r][0], g_reg[r][1], g_reg[r][2], g_reg[r][3]};
        if (do_bias) bsum[r][0] += (g_reg[r][0] + g_reg[r][1]) + (g_reg[r][2] + g_reg[r][3]);
      }
    }
  };

  const int wr = (wv >> 1) * (BE / 2), wc = (wv & 1) * (BKK / 2);
  const int r32 = lane & 31, half = lane >> 5;
  f32x16 acc[TI][TJ];
  zero_acc(acc);

  if (c_begin < c_end) {
    load_stage(c_begin);
    store_stage(0);
    __syncthreads();
    for (int ch = c_begin; ch < c_end; ++ch) {
      const int buf = (ch - c_begin) & 1;
      if (ch + 1 < c_end) load_stage(ch + 1);
      mfma_stage<false>(Gs[buf], As[buf], wr, wc, r32, half, acc);
      if (ch + 1 < c_end) store_stage(buf ^ 1);
      __syncthreads();
    }
  }

  // ---- this split's tile: rows e, columns kk (lanes along kk: 128-byte row segments)
  float* dst = wout + (int64_t)split * g.E * g.K;
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int kk = kk0 + wc + j * 32 + r32;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int e = e0 + wr + i * 32 + acc_row(v, half);
        if (e < g.E && kk < g.K) dst[(int64_t)e * g.K + kk] = acc[i][j][v];
      }
    }

  // ---- bias partials: the threads' sums meet in LDS (the last barrier of the loop has passed) and are added in slot order
  if (do_bias) {
    float* red = &Gs[0][0][0];                           // BE x slots floats, slots <= 16
    if constexpr (NHWC) {
#pragma unroll
      for (int r = 0; r < kGLoads; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(((tid + r * kThreads) / BR) * 4 + q) * BR + tid % BR] = bsum[r][q];
      __syncthreads();
      if (tid < BE && e0 + tid < g.E) {
        float t = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < BR; ++s2) t += red[tid * BR + s2];
        bout[(int64_t)split * g.E + e0 + tid] = t;
      }
    } else {
#pragma unroll
      for (int r = 0; r < kGLoads; ++r) red[((tid + r * kThreads) / 4) * 4 + tid % 4] = bsum[r][0];
      __syncthreads();
      if (tid < BE && e0 + tid < g.E) {
        const float t = (red[tid * 4] + red[tid * 4 + 1]) + (red[tid * 4 + 2] + red[tid * 4 + 3]);
        bout[(int64_t)split * g.E + e0 + tid] = t;
      }
    }
  }
}

// grad_bias alone: grid (E / 64, splits), the m range of each split as in patch_wgrad; a thread sums one channel over every
// fourth patch of the range, the four partial sums are added in order.
template <bool NHWC>
__global__ void __launch_bounds__(kThreads)
patch_colsum(const float* __restrict__ gout, Geom g, int splits, float* __restrict__ bout) {
  __shared__ float red[kThreads];
  const int tid = threadIdx.x;
  const int e_l = NHWC ? tid % 64 : tid / 4, q = NHWC ? tid / 64 : tid % 4;
  const int e = blockIdx.x * 64 + e_l, split = blockIdx.y;
  const long long chunks = ((long long)g.M + BR - 1) / BR;
  const int m_begin = (int)(chunks * split / splits) * BR;
  const int c_end = (int)(chunks * (split + 1) / splits);
  const int m_end = c_end * BR < g.M ? c_end * BR : g.M;
  const int HpWp = g.Hp * g.Wp;
  float s = 0.f;
  if (e < g.E) {
    for (int m = m_begin + q; m < m_end; m += 4) {
      const int b = m / HpWp, sp = m - b * HpWp;
      s += NHWC ? gout[(int64_t)m * g.E + e] : gout[((int64_t)b * g.E + e) * HpWp + sp];
    }
  }
  red[e_l * 4 + q] = s;
  __syncthreads();
  const int e_out = (int)blockIdx.x * 64 + tid;
  if (tid < 64 && e_out < g.E)
    bout[(int64_t)split * g.E + e_out] = (red[tid * 4] + red[tid * 4 + 1]) + (red[tid * 4 + 2] + red[tid * 4 + 3]);
}

// grad_weight / grad_bias = the splits' slabs added in split order (eight loads in flight, then their sums in order)
__global__ void __launch_bounds__(kThreads)
wgrad_reduce(const float* __restrict__ wparts, int splits, int64_t wtotal, float* __restrict__ grad_weight,
             const float* __restrict__ bparts, int E, float* __restrict__ grad_bias) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < wtotal + E; idx += (int64_t)gridDim.x * blockDim.x) {
    const bool is_w = idx < wtotal;
    if (is_w ? !grad_weight : !grad_bias) continue;
    const float* src = is_w ? wparts + idx : bparts + (idx - wtotal);
    const int64_t stride = is_w ? wtotal : E;
    float s = 0.f;
    int k = 0;
    for (; k + 8 <= splits; k += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(k + u) * stride];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; k < splits; ++k) s += src[(int64_t)k * stride];
    if (is_w) grad_weight[idx] = s;
    else grad_bias[idx - wtotal] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// grid (m tiles, kk tiles).  Ws[kk][16 e] (W is [E][K]: loaded along kk, stored transposed), Gs[m][16 e].
template <int KS, bool NHWC, int BKK, int BM>
__global__ void __launch_bounds__(kThreads, 2)
patch_dgrad(const float* __restrict__ w, const float* __restrict__ gout, Geom g, float* __restrict__ gx) {
  constexpr int kWLoads = BKK * BR / 4 / kThreads;     // 4 consecutive kk of one e
  constexpr int kGLoads = NHWC ? BM * BR / 4 / kThreads : BM * BR / kThreads;
  static_assert(kWLoads >= 1 && kGLoads >= 1, "tile");
  constexpr int TI = BKK / 64, TJ = BM / 64;
  __shared__ __attribute__((aligned(16))) float Ws[2][BKK][kPitch];
  __shared__ __attribute__((aligned(16))) float Gs[2][BM][kPitch];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m0 = blockIdx.x * BM, kk0 = blockIdx.y * BKK;
  const int HpWp = g.Hp * g.Wp;

  // NCHW G items: patch row tid % BM (the same for all items), channel (tid + 256 r) / BM -- lanes along the patches
  int64_t g_base = 0;
  bool g_mok = true;
  if constexpr (!NHWC) {
    const int m = m0 + tid % BM;
    g_mok = m < g.M;
    const int mc = g_mok ? m : 0;
    const int b = mc / HpWp, sp = mc - b * HpWp;
    g_base = (int64_t)b * g.E * HpWp + sp;
  }

  float w_reg[kWLoads][4];
  float g_reg[kGLoads][NHWC ? 4 : 1];
  auto load_stage = [&](int st) {
    const int er0 = st * BR;
#pragma unroll
    for (int r = 0; r < kWLoads; ++r) {
      const int i = tid + r * kThreads;
      const int kq = i % (BKK / 4), erow = i / (BKK / 4);
      const int e = er0 + erow, kk = kk0 + kq * 4;   // K % 16 == 0: a group of 4 is in range or not at all
      const float* p = w + (int64_t)e * g.K + kk;
      const bool ok = e < g.E && kk < g.K;
#pragma unroll
      for (int q = 0; q < 4; ++q) w_reg[r][q] = ok ? p[q] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < kGLoads; ++r) {
      const int i = tid + r * kThreads;
      if constexpr (NHWC) {
        const int eq = i % 4, mrow = i / 4;
        const int m = m0 + mrow, e = er0 + eq * 4;
        const float* p = gout + (int64_t)m * g.E + e;
        if (m < g.M && e + 3 < g.E) {
#pragma unroll
          for (int q = 0; q < 4; ++q) g_reg[r][q] = p[q];
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) g_reg[r][q] = (m < g.M && e + q < g.E) ? p[q] : 0.f;
        }
      } else {
        const int e = er0 + i / BM;
        g_reg[r][0] = (g_mok && e < g.E) ? gout[g_base + (int64_t)e * HpWp] : 0.f;
      }
    }
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int r = 0; r < kWLoads; ++r) {
      const int i = tid + r * kThreads;
      const int kq = i % (BKK / 4), erow = i / (BKK / 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) Ws[buf][kq * 4 + q][erow] = w_reg[r][q];
    }
#pragma unroll
    for (int r = 0; r < kGLoads; ++r) {
      const int i = tid + r * kThreads;
      if constexpr (NHWC) {
        const int eq = i % 4, mrow = i / 4;
        *reinterpret_cast<f32x4*>(&Gs[buf][mrow][eq * 4]) = f32x4{g_reg[r][0], g_reg[r][1], g_reg[r][2], g_reg[r][3]};
      } else {
        Gs[buf][i % BM][i / BM] = g_reg[r][0];
      }
    }
  };

  const int wr = (wv >> 1) * (BKK / 2), wc = (wv & 1) * (BM / 2);
  const int r32 = lane & 31, half = lane >> 5;
  f32x16 acc[TI][TJ];
  zero_acc(acc);

  const int NS = (g.E + BR - 1) / BR;
  load_stage(0);
  store_stage(0);
  __syncthreads();
  for (int st = 0; st < NS; ++st) {
    const int buf = st & 1;
    if (st + 1 < NS) load_stage(st + 1);
    mfma_stage<false>(Ws[buf], Gs[buf], wr, wc, r32, half, acc);
    if (st + 1 < NS) store_stage(buf ^ 1);
    __syncthreads();
  }

  // ---- scatter: rows kk, columns m.  For a fixed register, the lanes of a half-wave are 32 consecutive patches
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int m = m0 + wc + j * 32 + r32;
    if (m >= g.M) continue;
    const int64_t base = patch_base<KS>(m, g);
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int kk = kk0 + wr + i * 32 + acc_row(v, half);
        if (kk < g.K) {
          const int c = kk / (KS * KS), rr = kk % (KS * KS);
          gx[base + ((int64_t)c * g.H + rr / KS) * g.W + rr % KS] = acc[i][j][v];
        }
      }
  }
}

// zeros of the pixels no patch covers: per (b, c) plane the right strip (rows < Hc, columns >= Wc) then the bottom rows
__global__ void __launch_bounds__(kThreads)
zero_remainder(Geom g, int KS, float* __restrict__ gx) {
  const int Hc = g.Hp * KS, Wc = g.Wp * KS;
  const int64_t strip = (int64_t)Hc * (g.W - Wc), per_plane = strip + (int64_t)(g.H - Hc) * g.W;
  const int64_t total = (int64_t)g.B * g.C * per_plane;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t plane = idx / per_plane, r = idx - plane * per_plane;
    int y, xx;
    if (r < strip) {
      y = (int)(r / (g.W - Wc));
      xx = Wc + (int)(r - (int64_t)y * (g.W - Wc));
    } else {
      const int64_t r2 = r - strip;
      y = Hc + (int)(r2 / g.W);
      xx = (int)(r2 - (int64_t)(y - Hc) * g.W);
    }
    gx[(plane * g.H + y) * g.W + xx] = 0.f;
  }
}

template <int KS, int BE, int BKK>
static void launch_wgrad_t(const float* x, const float* gout, const Geom& g, int channels_last, int splits, float* wout,
                           float* bout, hipStream_t st) {
  const int groups = ((g.E + BE - 1) / BE) * ((g.K + BKK - 1) / BKK);
  dim3 grid((unsigned)groups, (unsigned)splits);
  if (channels_last)
    hipLaunchKernelGGL((patch_wgrad<KS, true, BE, BKK>), grid, dim3(kThreads), 0, st, x, gout, g, splits, wout, bout);
  else
    hipLaunchKernelGGL((patch_wgrad<KS, false, BE, BKK>), grid, dim3(kThreads), 0, st, x, gout, g, splits, wout, bout);
}

template <int KS>
static void launch_wgrad(const float* x, const float* gout, const Geom& g, int channels_last, int splits, float* wout,
                         float* bout, hipStream_t st) {
  if (wgrad_small(g.E, g.K)) launch_wgrad_t<KS, 64, 64>(x, gout, g, channels_last, splits, wout, bout, st);
  else launch_wgrad_t<KS, 128, 128>(x, gout, g, channels_last, splits, wout, bout, st);
}

template <int KS, int BKK, int BM>
static void launch_dgrad_t(const float* w, const float* gout, const Geom& g, int channels_last, float* gx, hipStream_t st) {
  dim3 grid((unsigned)((g.M + BM - 1) / BM), (unsigned)((g.K + BKK - 1) / BKK));
  if (channels_last) hipLaunchKernelGGL((patch_dgrad<KS, true, BKK, BM>), grid, dim3(kThreads), 0, st, w, gout, g, gx);
  else hipLaunchKernelGGL((patch_dgrad<KS, false, BKK, BM>), grid, dim3(kThreads), 0, st, w, gout, g, gx);
}

// rows of 64 kk when K is short (the stem's 48), else 128; 128 patches per workgroup
template <int KS>
static void launch_dgrad(const float* w, const float* gout, const Geom& g, int channels_last, float* gx, hipStream_t st) {
  if (g.K <= 64) launch_dgrad_t<KS, 64, 128>(w, gout, g, channels_last, gx, st);
  else launch_dgrad_t<KS, 128, 128>(w, gout, g, channels_last, gx, st);
}

}  // namespace patch_embed_bwd

extern "C" {

// the checks every entry point shares: 0 and the geometry, or a negative PATCH_EMBED_ERR_* (message set)
static int patch_bwd_geometry(int batch, int in_chans, int height, int width, int embed_dim, int patch, patch_embed_bwd::Geom* g) {
  if (batch < 0 || in_chans <= 0 || height <= 0 || width <= 0 || embed_dim <= 0 || patch <= 0)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "patch_embed backward: bad dimensions");
  if (patch != 2 && patch != 4 && patch != 8 && patch != 16)
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "patch_embed backward: patch size must be 2, 4, 8 or 16");
  const long long K = (long long)in_chans * patch * patch;
  if (K % patch_embed_bwd::BR != 0)
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "patch_embed backward: in_chans * patch^2 must be a multiple of 16");
  const long long Hp = height / patch, Wp = width / patch, M = (long long)batch * Hp * Wp;
  if (M >= (1ll << 31) - 256 || K >= (1ll << 31) || (long long)embed_dim * K >= (1ll << 31) ||
      (long long)batch * in_chans * height * width >= (1ll << 40) || (long long)embed_dim * M >= (1ll << 40) ||
      msda::ceil_div(K, 64ll) > 65535)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "patch_embed backward: problem too large");
  g->B = batch; g->C = in_chans; g->H = height; g->W = width; g->E = embed_dim;
  g->Hp = (int)Hp; g->Wp = (int)Wp; g->M = (int)M; g->K = (int)K;
  return 0;
}

size_t patch_embed_hip_backward_workspace_bytes(int batch, int in_chans, int height, int width, int embed_dim, int patch) {
  patch_embed_bwd::Geom g;
  if (batch < 0 || in_chans <= 0 || height <= 0 || width <= 0 || embed_dim <= 0 || patch <= 0) return 0;
  if (patch != 2 && patch != 4 && patch != 8 && patch != 16) return 0;
  if (((long long)in_chans * patch * patch) % patch_embed_bwd::BR != 0) return 0;
  if (patch_bwd_geometry(batch, in_chans, height, width, embed_dim, patch, &g) != 0) return 0;
  return patch_embed_bwd::layout(g.M, g.E, g.K).total;
}

int patch_embed_hip_backward_f32(const float* x, const float* weight, const float* grad_out, int batch, int in_chans,
                                 int height, int width, int embed_dim, int patch, int channels_last,
                                 float* grad_x, float* grad_weight, float* grad_bias,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  using namespace patch_embed_bwd;
  Geom g;
  int rc = patch_bwd_geometry(batch, in_chans, height, width, embed_dim, patch, &g);
  if (rc) return rc;
  if (!grad_x && !grad_weight && !grad_bias) return 0;
  const bool has_patches = g.M > 0, has_pixels = (long long)batch * in_chans * height * width > 0;
  const bool params = grad_weight || grad_bias;
  if ((has_patches && !grad_out) || (grad_weight && has_patches && !x) || (grad_x && has_patches && !weight))
    return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "patch_embed backward: null pointer argument");
  const Layout l = layout(g.M, g.E, g.K);
  if (params && has_patches) {
    if (!workspace) return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "patch_embed backward: null pointer argument");
    if (workspace_bytes < l.total)
      return msda::set_error(PATCH_EMBED_ERR_WORKSPACE,
                             "patch_embed backward: workspace smaller than patch_embed_hip_backward_workspace_bytes");
  }
  hipStream_t st = (hipStream_t)stream;

  if (!has_patches) {   // the gradients of a sum over no patches; every pixel of grad_x is a remainder pixel
    if (grad_weight && hipMemsetAsync(grad_weight, 0, (size_t)g.E * g.K * sizeof(float), st) != hipSuccess) return msda::launch_status();
    if (grad_bias && hipMemsetAsync(grad_bias, 0, (size_t)g.E * sizeof(float), st) != hipSuccess) return msda::launch_status();
  }
  if (grad_x && has_pixels && (g.H % patch != 0 || g.W % patch != 0 || !has_patches)) {
    const int64_t per_plane = (int64_t)g.H * g.W - (int64_t)g.Hp * patch * g.Wp * patch;
    long long blocks = ((long long)batch * in_chans * per_plane + kThreads - 1) / kThreads;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(zero_remainder, dim3((unsigned)blocks), dim3(kThreads), 0, st, g, patch, grad_x);
    if ((rc = msda::launch_status())) return rc;
  }
  if (!has_patches) return 0;

  if (grad_x) {
    switch (patch) {
      case 2: launch_dgrad<2>(weight, grad_out, g, channels_last, grad_x, st); break;
      case 4: launch_dgrad<4>(weight, grad_out, g, channels_last, grad_x, st); break;
      case 8: launch_dgrad<8>(weight, grad_out, g, channels_last, grad_x, st); break;
      default: launch_dgrad<16>(weight, grad_out, g, channels_last, grad_x, st); break;
    }
    if ((rc = msda::launch_status())) return rc;
  }
  if (!params) return 0;

  char* ws = static_cast<char*>(workspace);
  const bool direct = l.splits == 1;   // one split: the tiles are the gradients
  float* wout = direct ? grad_weight : reinterpret_cast<float*>(ws + l.wparts);
  float* bout = direct ? grad_bias : reinterpret_cast<float*>(ws + l.bparts);
  if (grad_weight) {
    float* b_arg = grad_bias ? bout : nullptr;
    switch (patch) {
      case 2: launch_wgrad<2>(x, grad_out, g, channels_last, l.splits, wout, b_arg, st); break;
      case 4: launch_wgrad<4>(x, grad_out, g, channels_last, l.splits, wout, b_arg, st); break;
      case 8: launch_wgrad<8>(x, grad_out, g, channels_last, l.splits, wout, b_arg, st); break;
      default: launch_wgrad<16>(x, grad_out, g, channels_last, l.splits, wout, b_arg, st); break;
    }
  } else {
    dim3 grid((unsigned)msda::ceil_div(g.E, 64), (unsigned)l.splits);
    if (channels_last) hipLaunchKernelGGL(patch_colsum<true>, grid, dim3(kThreads), 0, st, grad_out, g, l.splits, bout);
    else hipLaunchKernelGGL(patch_colsum<false>, grid, dim3(kThreads), 0, st, grad_out, g, l.splits, bout);
  }
  if ((rc = msda::launch_status())) return rc;
  if (!direct) {
    const int64_t wtotal = grad_weight ? (int64_t)g.E * g.K : 0;
    long long blocks = (wtotal + g.E + kThreads - 1) / kThreads;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(wgrad_reduce, dim3((unsigned)blocks), dim3(kThreads), 0, st, reinterpret_cast<const float*>(ws + l.wparts),
                       l.splits, wtotal, grad_weight, reinterpret_cast<const float*>(ws + l.bparts), g.E, grad_bias);
    rc = msda::launch_status();
  }
  return rc;
}

}  // extern "C"
