// Encoder input preparation (include/dynmask_hip.h: encprep_hip_*): what stands between the backbone's features and the first
// encoder layer (ddetrs_dn.py:117-143, deformable_transformer_dino.py:181-201 and :289-301, position_encoding.py:36-56), in four
// launches that each cover every level of the call through a by-value level table:
//   masks     the levels' padding masks by PyTorch's legacy `nearest` rule from the image mask, flattened; their cumulative counts
//             (y_embed, x_embed) and column / row totals; valid_ratios.  Integer counts, one thread per column, one wave per row.
//   pos       one wave per token: the 256 channels of the sine embedding plus level_embed as one 1 KB row of 16-byte stores, and
//             the token's reference points.
//   gn_stats  float64 partial sums of x and x * x of one slice of a GroupNorm group (8 channels = one contiguous run of NCHW).
//   gn_apply  combines a (batch, level)'s partial sums in a fixed order, normalises a tile of 256 channels x 32 pixels in float64
//             and writes it, transposed through LDS, as token rows of src_flatten with 16-byte stores.
// No atomics; every sum has a fixed order: the outputs are the same bits on every call.
#include "../../include/dynmask_hip.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "launch_glue.hpp"
#include "wave_ops.hpp"

namespace encprep {

constexpr int kMaxLevels = ENCPREP_HIP_MAX_LEVELS;
constexpr int kC = ENCPREP_HIP_CHANNELS;          // d_model
constexpr int kGroups = ENCPREP_HIP_GROUPS;       // GroupNorm(32, 256): 8 adjacent channels a group
constexpr int kGroupC = kC / kGroups;
constexpr int kPosFeats = kC / 2;                 // num_pos_feats of PositionEmbeddingSine
constexpr int kP = ENCPREP_HIP_PIXEL_TILE;        // pixels of a gn_apply tile
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxParts = 8;                      // slices of a group's run, each a workgroup of gn_stats
constexpr int kPartFloat4 = 1024;                 // a slice is at least this many float4 (but for the last)
constexpr int kTileStride = kC + 4;               // floats of a tile row in LDS: 16-byte aligned rows an odd number of 16-byte slots apart
static_assert(kC == 256 && kGroupC == 8 && kP == 32 && kThreads == 256, "the index arithmetic below is written for these");

// By value in the kernel arguments.  Only ever indexed by constants (pick() below), so it stays in scalar registers.
struct Levels {
  int n;
  int H[kMaxLevels], W[kMaxLevels];
  int sH[kMaxLevels], sW[kMaxLevels];            // the level the mask is resized from; 0: from the image mask itself
  int start[kMaxLevels];                         // first token
  int tot[kMaxLevels];                           // first of the level's W column totals, then H row totals
  int parts[kMaxLevels];                         // gn_stats slices of a group
  int item[kMaxLevels];                          // first gn_stats work item: item + ((b * 32 + g) * parts + part)
  int tile[kMaxLevels];                          // first gn_apply tile: tile + b * ceil(HW / kP) + t
  int S, T;                                      // tokens, totals per image
};
struct Planes { const float* p[kMaxLevels]; };
struct Scalars { float v[kMaxLevels]; };

__device__ __forceinline__ int pick(const int (&a)[kMaxLevels], int l) {
  int v = a[0];
#pragma unroll
  for (int k = 1; k < kMaxLevels; ++k) v = (l == k) ? a[k] : v;
  return v;
}
__device__ __forceinline__ const float* pick(const Planes& a, int l) {
  const float* v = a.p[0];
#pragma unroll
  for (int k = 1; k < kMaxLevels; ++k) v = (l == k) ? a.p[k] : v;
  return v;
}
__device__ __forceinline__ float pick(const Scalars& a, int l) {
  float v = a.v[0];
#pragma unroll
  for (int k = 1; k < kMaxLevels; ++k) v = (l == k) ? a.v[k] : v;
  return v;
}
// the last level whose first entry of `first` is not above i
__device__ __forceinline__ int level_of(const Levels& lv, const int (&first)[kMaxLevels], int i) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < kMaxLevels; ++k) l = (k < lv.n && i >= first[k]) ? k : l;
  return l;
}

// F.interpolate(mode='nearest'): the scale is a float and so is the product
__device__ __forceinline__ int nearest(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  return min((int)floorf((float)dst * scale), in - 1);
}

struct MaskGeom { int H, W, sH, sW, Hi, Wi; };
__device__ __forceinline__ int mask_row(const MaskGeom& g, int y) {
  return g.sH > 0 ? nearest(nearest(y, g.sH, g.H), g.Hi, g.sH) : nearest(y, g.Hi, g.H);
}
__device__ __forceinline__ int mask_col(const MaskGeom& g, int x) {
  return g.sW > 0 ? nearest(nearest(x, g.sW, g.W), g.Wi, g.sW) : nearest(x, g.Wi, g.W);
}

// grid (level, image).  y_embed / x_embed are the reference's cumsums of ~mask, exact integers held as floats.
__global__ __launch_bounds__(kThreads) void masks(const unsigned char* __restrict__ image_mask, int Hi, int Wi, Levels lv,
                                                   unsigned char* __restrict__ mask_flatten, float* __restrict__ valid_ratios,
                                                   float* __restrict__ yx_embed, float* __restrict__ totals) {
  const int l = blockIdx.x, b = blockIdx.y;
  const MaskGeom g{pick(lv.H, l), pick(lv.W, l), pick(lv.sH, l), pick(lv.sW, l), Hi, Wi};
  const unsigned char* img = image_mask + (size_t)b * Hi * Wi;
  const size_t tok0 = (size_t)b * lv.S + pick(lv.start, l);
  float* tot = totals + (size_t)b * lv.T + pick(lv.tot, l);
  float* vr = valid_ratios + ((size_t)b * lv.n + l) * 2;

  for (int x = threadIdx.x; x < g.W; x += kThreads) {        // a column: mask bytes, y_embed, the column's total
    const int xi = mask_col(g, x);
    int cnt = 0;
    for (int y = 0; y < g.H; ++y) {
      const unsigned char m = img[(size_t)mask_row(g, y) * Wi + xi] != 0;
      cnt += 1 - m;
      const size_t t = tok0 + (size_t)y * g.W + x;
      mask_flatten[t] = m;
      yx_embed[2 * t] = (float)cnt;
    }
    tot[x] = (float)cnt;
    if (x == 0) vr[1] = (float)cnt / (float)g.H;               // get_valid_ratio: the first column's count over H
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int y = wave; y < g.H; y += kWaves) {                   // a row: x_embed by a wave scan, the row's total
    const int yi = mask_row(g, y);
    int carry = 0;
    for (int x0 = 0; x0 < g.W; x0 += 64) {
      const int x = x0 + lane;
      const bool valid = x < g.W && img[(size_t)yi * Wi + mask_col(g, min(x, g.W - 1))] == 0;
      const unsigned long long bits = __ballot(valid);
      if (x < g.W) yx_embed[2 * (tok0 + (size_t)y * g.W + x) + 1] = (float)(carry + __popcll(bits & (~0ull >> (63 - lane))));
      carry += __popcll(bits);
    }
    if (lane == 0) {
      tot[g.W + y] = (float)carry;
      if (y == 0) vr[0] = (float)carry / (float)g.W;           // the first row's count over W
    }
  }
}

// A wave per token.  Lanes 0 .. 31 hold the 128 channels of pos_y, lanes 32 .. 63 those of pos_x, four adjacent channels each:
// two (sin, cos) pairs, a pair sharing its dim_t.  The argument is formed as the reference forms it, one rounding per operation.
__global__ __launch_bounds__(kThreads) void pos(const float* __restrict__ yx_embed, const float* __restrict__ totals,
                                                 const float* __restrict__ valid_ratios, const float* __restrict__ level_embed,
                                                 const float* __restrict__ dim_t, Levels lv, int batch, float scale, float eps,
                                                 float* __restrict__ lvl_pos_embed, float* __restrict__ reference_points) {
  const int lane = threadIdx.x & 63;
  const long long token = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (token >= (long long)batch * lv.S) return;
  const int b = (int)(token / lv.S), s = (int)(token % lv.S);
  const int l = level_of(lv, lv.start, s);
  const int H = pick(lv.H, l), W = pick(lv.W, l), local = s - pick(lv.start, l);
  const int y = local / W, x = local % W;
  const float* tot = totals + (size_t)b * lv.T + pick(lv.tot, l);
  const bool is_y = lane < 32;
  const float cnt = yx_embed[2 * (size_t)token + (is_y ? 0 : 1)];
  const float total = is_y ? tot[x] : tot[W + y];
  const float e = ((cnt - 0.5f) / (total + eps)) * scale;
  const int c = 4 * lane;
  const float4 le = *reinterpret_cast<const float4*>(level_embed + (size_t)l * kC + c);
  const float d0 = dim_t[c & (kPosFeats - 1)], d1 = dim_t[(c + 2) & (kPosFeats - 1)];
  float s0, c0, s1, c1;
  sincosf(e / d0, &s0, &c0);
  sincosf(e / d1, &s1, &c1);
  float4 out;
  out.x = s0 + le.x; out.y = c0 + le.y; out.z = s1 + le.z; out.w = c1 + le.w;
  *reinterpret_cast<float4*>(lvl_pos_embed + (size_t)token * kC + c) = out;

  if (lane < 2 * lv.n) {                                       // get_reference_points: [b, s, level, (x, y)]
    const int to = lane >> 1, xy = lane & 1;
    const float* vr = valid_ratios + (size_t)b * lv.n * 2;
    const float base = xy == 0 ? ((float)x + 0.5f) / (vr[2 * l] * (float)W) : ((float)y + 0.5f) / (vr[2 * l + 1] * (float)H);
    reference_points[(size_t)token * lv.n * 2 + lane] = base * vr[2 * to + xy];
  }
}

// A workgroup per (level, image, group, slice): the slice's sums of x and x * x in float64, lanes, then waves, in a fixed order.
__global__ __launch_bounds__(kThreads) void gn_stats(Planes xs, Levels lv, double* __restrict__ partials) {
  const int item = blockIdx.x;
  const int l = level_of(lv, lv.item, item);
  const int parts = pick(lv.parts, l), local = item - pick(lv.item, l);
  const int part = local % parts, bg = local / parts;           // bg = b * 32 + g: the group's run starts at bg * 8 * HW
  const size_t n4 = (size_t)pick(lv.H, l) * pick(lv.W, l) * (kGroupC / 4);
  const float4* run = reinterpret_cast<const float4*>(pick(xs, l)) + (size_t)bg * n4;
  const size_t per = (n4 + parts - 1) / parts;
  const size_t lo = per * part, hi = lo + per < n4 ? lo + per : n4;
  double s = 0.0, q = 0.0;
  for (size_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    const float4 v = run[i];
    const double a = v.x, bb = v.y, c = v.z, d = v.w;
    s += (a + bb) + (c + d);
    q += (a * a + bb * bb) + (c * c + d * d);
  }
  s = wave_ops::wave_sum(s);
  q = wave_ops::wave_sum(q);
  __shared__ double red[kWaves][2];
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s; red[threadIdx.x >> 6][1] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ts = red[0][0], tq = red[0][1];
    for (int w = 1; w < kWaves; ++w) { ts += red[w][0]; tq += red[w][1]; }
    partials[2 * (size_t)item] = ts;
    partials[2 * (size_t)item + 1] = tq;
  }
}

// A workgroup per (level, image, tile of 32 pixels).  A half wave loads 32 adjacent pixels of a channel (4-byte loads: a channel
// row of NCHW starts at any multiple of 4 bytes), a thread four adjacent channels of its pixel, which it normalises and writes to
// LDS as one 16-byte slot of the pixel's row; a wave then reads a row back and stores it as the token's 1 KB of src_flatten.
__global__ __launch_bounds__(kThreads) void gn_apply(Planes xs, Planes weights, Planes biases, Levels lv, Scalars eps_all,
                                                      const double* __restrict__ partials, float* __restrict__ src_flatten,
                                                      float* __restrict__ mean_out, float* __restrict__ rstd_out, int batch) {
  __shared__ __attribute__((aligned(16))) float tile[kP * kTileStride];
  __shared__ double stat[kGroups][2];
  const int l = level_of(lv, lv.tile, blockIdx.x);
  const int HW = pick(lv.H, l) * pick(lv.W, l);
  const int tiles = (HW + kP - 1) / kP, local = blockIdx.x - pick(lv.tile, l);
  const int b = local / tiles, p0 = (local % tiles) * kP;

  if (threadIdx.x < kGroups) {                                  // the group's slices, first to last
    const int parts = pick(lv.parts, l), g = threadIdx.x;
    const double* part = partials + 2 * ((size_t)pick(lv.item, l) + (size_t)(b * kGroups + g) * parts);
    double s = part[0], q = part[1];
    for (int k = 1; k < parts; ++k) { s += part[2 * k]; q += part[2 * k + 1]; }
    const double n = (double)HW * kGroupC;
    const double mean = s / n;
    const double var = fmax(q / n - mean * mean, 0.0);
    const double rstd = 1.0 / sqrt(var + (double)pick(eps_all, l));
    stat[g][0] = mean;
    stat[g][1] = rstd;
    if (p0 == 0) {
      const size_t o = ((size_t)b * lv.n + l) * kGroups + g;
      mean_out[o] = (float)mean;
      rstd_out[o] = (float)rstd;
    }
  }
  __syncthreads();

  const float* x = pick(xs, l) + (size_t)b * kC * HW;
  const float* w = pick(weights, l);
  const float* bs = pick(biases, l);
  const int px = threadIdx.x & (kP - 1), half = threadIdx.x / kP;          // 8 half waves
  const bool live = p0 + px < HW;
#pragma unroll 4
  for (int quad = half; quad < kC / 4; quad += kThreads / kP) {
    const int c = 4 * quad;
    const float* src = x + (size_t)c * HW + p0 + px;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = live ? src[(size_t)k * HW] : 0.f;
    const double mean = stat[c / kGroupC][0], rstd = stat[c / kGroupC][1];
    float4 o;
    o.x = (float)(((double)v[0] - mean) * rstd * (double)w[c] + (double)bs[c]);
    o.y = (float)(((double)v[1] - mean) * rstd * (double)w[c + 1] + (double)bs[c + 1]);
    o.z = (float)(((double)v[2] - mean) * rstd * (double)w[c + 2] + (double)bs[c + 2]);
    o.w = (float)(((double)v[3] - mean) * rstd * (double)w[c + 3] + (double)bs[c + 3]);
    *reinterpret_cast<float4*>(&tile[px * kTileStride + c]) = o;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* dst = src_flatten + ((size_t)b * lv.S + pick(lv.start, l) + p0) * kC;
  const int rows = min(kP, HW - p0);
  for (int r = wave; r < rows; r += kWaves)
    *reinterpret_cast<float4*>(dst + (size_t)r * kC + 4 * lane) = *reinterpret_cast<const float4*>(&tile[r * kTileStride + 4 * lane]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The level table from the caller's [n_levels, 3] host ints (H, W, source level or -1 for the image mask).  0, or the refusal.
static int make_levels(const char* who, int batch, const int* levels, int n_levels, Levels* out, bool* empty) {
  static thread_local char msg[160];
  auto refuse = [&](int code, const char* what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return msda::set_error(code, msg);
  };
  *empty = true;
  if (batch < 0 || n_levels < 0) return refuse(DYNMASK_ERR_BAD_DIMS, "bad dimensions");
  if (n_levels > kMaxLevels) return refuse(DYNMASK_ERR_UNSUPPORTED, "at most 8 levels");
  if (batch == 0 || n_levels == 0) return 0;
  if (!levels) return refuse(DYNMASK_ERR_NULL_POINTER, "null pointer argument");
  Levels lv = {};
  lv.n = n_levels;
  long long S = 0, T = 0, items = 0, tiles = 0;
  for (int l = 0; l < n_levels; ++l) {
    const int H = levels[3 * l], W = levels[3 * l + 1], src = levels[3 * l + 2];
    if (H <= 0 || W <= 0 || H > (1 << 15) || W > (1 << 15)) return refuse(DYNMASK_ERR_BAD_DIMS, "bad dimensions");
    if (src >= l || src < -1 || (src >= 0 && levels[3 * src + 2] != -1))
      return refuse(DYNMASK_ERR_BAD_DIMS, "a level's mask source is the image (-1) or an earlier level whose source is the image");
    lv.H[l] = H; lv.W[l] = W;
    lv.sH[l] = src >= 0 ? levels[3 * src] : 0;
    lv.sW[l] = src >= 0 ? levels[3 * src + 1] : 0;
    lv.start[l] = (int)S; lv.tot[l] = (int)T; lv.item[l] = (int)items; lv.tile[l] = (int)tiles;
    const long long n4 = (long long)H * W * (kGroupC / 4);
    lv.parts[l] = (int)std::min<long long>(kMaxParts, std::max<long long>(1, n4 / kPartFloat4));
    S += (long long)H * W; T += H + W;
    items += (long long)batch * kGroups * lv.parts[l];
    tiles += (long long)batch * msda::ceil_div((long long)H * W, (long long)kP);
    if ((long long)batch * S * kC >= (1ll << 31) || items >= (1ll << 31)) return refuse(DYNMASK_ERR_BAD_DIMS, "problem too large");
  }
  lv.S = (int)S; lv.T = (int)T;
  *out = lv;
  *empty = false;
  return 0;
}

static int item_count(const Levels& lv, int batch) { return lv.item[lv.n - 1] + batch * kGroups * lv.parts[lv.n - 1]; }
static int tile_count(const Levels& lv, int batch) {
  return lv.tile[lv.n - 1] + batch * msda::ceil_div(lv.H[lv.n - 1] * lv.W[lv.n - 1], kP);
}

}  // namespace encprep

extern "C" {

static const char* g_encprep_last = "";

const char* encprep_hip_last_kernel(void) { return g_encprep_last; }

size_t encprep_hip_workspace_bytes(int batch, const int* levels, int n_levels) {
  encprep::Levels lv;
  bool empty;
  if (encprep::make_levels("encprep_workspace_bytes", batch, levels, n_levels, &lv, &empty) != 0 || empty) return 0;
  return (size_t)encprep::item_count(lv, batch) * 2 * sizeof(double);
}

int encprep_hip_masks_u8(const unsigned char* image_mask, int batch, int Hi, int Wi, const int* levels, int n_levels,
                         unsigned char* mask_flatten, float* valid_ratios, float* yx_embed, float* totals, void* stream) {
  encprep::Levels lv;
  bool empty;
  if (const int e = encprep::make_levels("encprep_masks", batch, levels, n_levels, &lv, &empty)) return e;
  if (empty) return 0;
  if (Hi <= 0 || Wi <= 0 || Hi > (1 << 15) || Wi > (1 << 15)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "encprep_masks: bad dimensions");
  if (!image_mask || !mask_flatten || !valid_ratios || !yx_embed || !totals)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "encprep_masks: null pointer argument");
  hipLaunchKernelGGL(encprep::masks, dim3((unsigned)n_levels, (unsigned)batch), dim3(encprep::kThreads), 0, (hipStream_t)stream,
                     image_mask, Hi, Wi, lv, mask_flatten, valid_ratios, yx_embed, totals);
  if (const int e = msda::launch_status()) return e;
  g_encprep_last = "encprep_masks";
  return 0;
}

int encprep_hip_pos_f32(const float* yx_embed, const float* totals, const float* valid_ratios, const float* level_embed,
                        const float* dim_t, int batch, const int* levels, int n_levels, int channels, float scale, float eps,
                        float* lvl_pos_embed, float* reference_points, void* stream) {
  encprep::Levels lv;
  bool empty;
  if (const int e = encprep::make_levels("encprep_pos", batch, levels, n_levels, &lv, &empty)) return e;
  if (channels != encprep::kC) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "encprep_pos: 256 channels (num_pos_feats 128) only");
  if (empty) return 0;
  if (!yx_embed || !totals || !valid_ratios || !level_embed || !dim_t || !lvl_pos_embed || !reference_points)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "encprep_pos: null pointer argument");
  if (!msda::aligned16({level_embed, lvl_pos_embed}))
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "encprep_pos: level_embed and lvl_pos_embed must be 16-byte aligned");
  const long long tokens = (long long)batch * lv.S;
  hipLaunchKernelGGL(encprep::pos, dim3((unsigned)msda::ceil_div(tokens, (long long)encprep::kWaves)), dim3(encprep::kThreads), 0,
                     (hipStream_t)stream, yx_embed, totals, valid_ratios, level_embed, dim_t, lv, batch, scale, eps, lvl_pos_embed,
                     reference_points);
  if (const int e = msda::launch_status()) return e;
  g_encprep_last = "encprep_pos";
  return 0;
}

int encprep_hip_gn_stats_f32(const float* const* x, int batch, const int* levels, int n_levels, int channels, int groups,
                             double* partials, size_t partial_bytes, void* stream) {
  encprep::Levels lv;
  bool empty;
  if (const int e = encprep::make_levels("encprep_gn_stats", batch, levels, n_levels, &lv, &empty)) return e;
  if (channels != encprep::kC || groups != encprep::kGroups)
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "encprep_gn_stats: GroupNorm(32, 256) only");
  if (empty) return 0;
  if (!x || !partials) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "encprep_gn_stats: null pointer argument");
  encprep::Planes xs = {};
  for (int l = 0; l < n_levels; ++l) {
    if (!x[l]) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "encprep_gn_stats: null pointer argument");
    if (!msda::aligned16({x[l]})) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "encprep_gn_stats: x must be 16-byte aligned");
    xs.p[l] = x[l];
  }
  const int items = encprep::item_count(lv, batch);
  if (partial_bytes < (size_t)items * 2 * sizeof(double) || !msda::aligned16({partials}))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "encprep_gn_stats: partials below encprep_hip_workspace_bytes or not 16-byte aligned");
  hipLaunchKernelGGL(encprep::gn_stats, dim3((unsigned)items), dim3(encprep::kThreads), 0, (hipStream_t)stream, xs, lv, partials);
  if (const int e = msda::launch_status()) return e;
  g_encprep_last = "encprep_gn_stats";
  return 0;
}

int encprep_hip_gn_apply_f32(const float* const* x, const float* const* weight, const float* const* bias, const float* eps,
                             const double* partials, size_t partial_bytes, int batch, const int* levels, int n_levels, int channels,
                             int groups, float* src_flatten, float* mean, float* rstd, void* stream) {
  encprep::Levels lv;
  bool empty;
  if (const int e = encprep::make_levels("encprep_gn_apply", batch, levels, n_levels, &lv, &empty)) return e;
  if (channels != encprep::kC || groups != encprep::kGroups)
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "encprep_gn_apply: GroupNorm(32, 256) only");
  if (empty) return 0;
  if (!x || !weight || !bias || !eps || !partials || !src_flatten || !mean || !rstd)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "encprep_gn_apply: null pointer argument");
  encprep::Planes xs = {}, ws = {}, bs = {};
  for (int l = 0; l < n_levels; ++l) {
    if (!x[l] || !weight[l] || !bias[l]) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "encprep_gn_apply: null pointer argument");
    xs.p[l] = x[l]; ws.p[l] = weight[l]; bs.p[l] = bias[l];
  }
  if (!msda::aligned16({src_flatten, partials}))
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "encprep_gn_apply: src_flatten and partials must be 16-byte aligned");
  if (partial_bytes < (size_t)encprep::item_count(lv, batch) * 2 * sizeof(double))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "encprep_gn_apply: partials below encprep_hip_workspace_bytes");
  encprep::Scalars eps_all = {};
  for (int l = 0; l < n_levels; ++l) {
    if (!(eps[l] > 0.f)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "encprep_gn_apply: eps must be positive");
    eps_all.v[l] = eps[l];
  }
  hipLaunchKernelGGL(encprep::gn_apply, dim3((unsigned)encprep::tile_count(lv, batch)), dim3(encprep::kThreads), 0, (hipStream_t)stream,
                     xs, ws, bs, lv, eps_all, partials, src_flatten, mean, rstd, batch);
  if (const int e = msda::launch_status()) return e;
  g_encprep_last = "encprep_gn_apply";
  return 0;
}

}  // extern "C"
