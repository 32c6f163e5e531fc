// Mask post-processing: the binarised, resized instance masks of an image, and the tracker's mask NMS -- see
// include/dynmask_hip.h (maskpost_binarize_hip_f32, maskpost_pack_hip_f32, maskpost_nms_hip_u32).
//
//   binarize  one workgroup per (instance, band of output rows, tile of 2048 output columns).  It first forms, in LDS, the
//             tile's column table (lower neighbour and weight of the low-resolution column every output column reads) and the
//             vertical blend of the two low-resolution rows every output row of the band reads; row and column indices are
//             thus formed once per row or column.  A lane then forms 16 consecutive output bytes (two LDS reads, the
//             horizontal blend, the sigmoid and the comparison per byte) and stores them with one 16-byte store, so a wave
//             writes 1 KiB of a row; the bytes before a row's first 16-byte boundary and after its last go out one by one.
//   pack      one workgroup per instance: a wave reads 64 consecutive logits, one ballot gives two words of the bit mask.
//   pairs     one wave per pair (i, j >= i) of packed masks: popcounts of the ANDed words, butterfly sum.
//   scan      one workgroup: the waves fill the suppression matrix (a ballot per 64 columns), wave 0 walks the masks in the
//             given order and ORs the rows of the masks it keeps into the removed-mask, as detpost::nms does.
//
// Compiled without contraction: every operation of a pinned expression rounds as one IEEE fp32 operation.  No atomics, fixed
// orders: bitwise repeatable.
#pragma clang fp contract(off)
#include "../../include/dynmask_hip.h"

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "launch_glue.hpp"
#include "msda_common.hpp"

namespace maskpost {

using msda::sigmoidf;
using wave_ops::shfl64;

constexpr int kThreads = 256;
constexpr int kTileW = 2048;                   // output columns of a workgroup: 8 B of column table each
constexpr int kMaxBand = 16;                   // output rows of a workgroup at most
constexpr int kBlendFloats = 8192;             // blended low-resolution rows of a band: 32 KB
constexpr int kMaxW = MASKPOST_HIP_MAX_WIDTH;
constexpr int kMaxN = MASKPOST_HIP_MAX_MASKS;
constexpr int kPackThreads = 512;
constexpr int kScanThreads = 1024;
constexpr int kMaxWords64 = kMaxN / 64;
constexpr int kScanLdsMax = (kMaxN * kMaxWords64 + kMaxWords64) * 8;      // the matrix and the removed-mask
static_assert(kMaxW <= kBlendFloats, "a band holds at least one blended row");
static_assert(kBlendFloats * 4 + kTileW * 8 <= 64 * 1024, "binarize stays under the LDS a launch gets without opting in");
static_assert(kScanLdsMax + 256 <= 160 * 1024 && kMaxN <= kScanThreads && kMaxWords64 <= 64, "one workgroup, a lane per mask word");

// F.interpolate(mode='nearest'): the product in fp32
__device__ __forceinline__ int nearest(int dst, float scale, int in) { return min((int)floorf(__fmul_rn((float)dst, scale)), in - 1); }

// bilinear, align_corners = False: lower neighbour and the weight of the upper one
__device__ __forceinline__ int source(int dst, float inv_stride, int size, float* weight) {
  const float s = fmaxf(((float)dst + 0.5f) * inv_stride - 0.5f, 0.f);
  const int lo = min((int)s, size - 1);
  *weight = s - (float)lo;
  return lo;
}

__device__ __forceinline__ unsigned pixel(const float* __restrict__ row, const int* __restrict__ cx0, const float* __restrict__ clx,
                                          int c, int wm1, float thres) {
  const int x0 = cx0[c];
  const float lx = clx[c];
  const float v = (1.f - lx) * row[x0] + lx * row[min(x0 + 1, wm1)];
  return sigmoidf(v) > thres ? 1u : 0u;
}

__global__ void __launch_bounds__(kThreads)
binarize(const float* __restrict__ logits, const long long* __restrict__ rows, int Q, int h, int w, float inv_stride, int crop_h,
         int crop_w, int out_h, int out_w, float scale_h, float scale_w, float thres, int band, int tile_cap, int xtiles,
         int ybands, unsigned char* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* blend = reinterpret_cast<float*>(smem);                   // [band][w]
  float* clx = blend + (size_t)band * w;                           // [tile_cap]
  int* cx0 = reinterpret_cast<int*>(clx + tile_cap);               // [tile_cap]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int xt = blockIdx.x % xtiles, yb = (blockIdx.x / xtiles) % ybands, inst = blockIdx.x / (xtiles * ybands);
  const int c0 = xt * kTileW, oy0 = yb * band;
  const int ncols = min(kTileW, out_w - c0), nrows = min(band, out_h - oy0);
  const long long q = rows[inst];
  const bool live = q >= 0 && q < Q;

  for (int c = tid; c < ncols; c += kThreads) {
    float lx;
    cx0[c] = source(nearest(c0 + c, scale_w, crop_w), inv_stride, w, &lx);
    clx[c] = lx;
  }
  const float* __restrict__ plane = logits + (live ? q : 0) * h * w;
  for (int r = wv; r < nrows; r += kThreads / 64) {
    float ly;
    const int y0 = source(nearest(oy0 + r, scale_h, crop_h), inv_stride, h, &ly), y1 = min(y0 + 1, h - 1);
    const float* __restrict__ a = plane + (size_t)y0 * w;
    const float* __restrict__ b = plane + (size_t)y1 * w;
    for (int x = lane; x < w; x += 64) blend[r * w + x] = live ? (1.f - ly) * a[x] + ly * b[x] : -1e30f;
  }
  __syncthreads();

  // a row's bytes of this tile: `head` bytes up to the first 16-byte boundary (chunk 0), then chunks of 16
  const int chunks = (ncols + 15) / 16 + 1;
  const int wm1 = w - 1;
  for (int item = tid; item < nrows * chunks; item += kThreads) {
    const int r = item / chunks, k = item - r * chunks;
    unsigned char* __restrict__ dst = out + ((long long)inst * out_h + oy0 + r) * out_w + c0;
    const int head = min((int)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15), ncols);
    const int cb = k == 0 ? 0 : head + 16 * (k - 1), ce = k == 0 ? head : min(cb + 16, ncols);
    const float* __restrict__ row = blend + r * w;
    if (k > 0 && ce - cb == 16) {
      msda::u32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned word = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) word |= pixel(row, cx0, clx, cb + 4 * j + e, wm1, thres) << (8 * e);
        v[j] = word;
      }
      *reinterpret_cast<msda::u32x4*>(dst + cb) = v;
    } else {
      for (int c = cb; c < ce; ++c) dst[c] = (unsigned char)pixel(row, cx0, clx, c, wm1, thres);
    }
  }
}

__global__ void __launch_bounds__(kPackThreads)
pack(const float* __restrict__ logits, const long long* __restrict__ rows, int Q, int hw, int words, unsigned* __restrict__ bits,
     int* __restrict__ area) {
  __shared__ int red[kPackThreads / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, inst = blockIdx.x;
  const long long q = rows[inst];
  const bool live = q >= 0 && q < Q;
  const float* __restrict__ src = logits + (live ? q : 0) * hw;
  unsigned* __restrict__ dst = bits + (long long)inst * words;
  int count = 0;
  for (int base = wv * 64; base < words * 32; base += kPackThreads) {       // wave-uniform; base / 32 is even
    const int k = base + lane;
    const bool on = live && k < hw && sigmoidf(src[k]) > 0.5f;
    const unsigned long long b = __ballot(on);
    count += __popcll(b);
    const int word = base / 32 + lane;
    if (lane < 2 && word < words) dst[word] = (unsigned)(b >> (32 * lane));
  }
  if (lane == 0) red[wv] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int k = 0; k < kPackThreads / 64; ++k) total += red[k];
    area[inst] = total;
  }
}

__global__ void __launch_bounds__(kThreads)
pairs(const unsigned* __restrict__ bits, int n, int words, int* __restrict__ inter) {
  const int lane = threadIdx.x & 63, i = blockIdx.y, j = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (j >= n || j < i) return;                 // wave-uniform
  const unsigned* __restrict__ a = bits + (long long)i * words;
  const unsigned* __restrict__ b = bits + (long long)j * words;
  int count = 0;
  for (int k = lane; k < words; k += 64) count += __popc(a[k] & b[k]);
  count = wave_ops::wave_sum(count);
  if (lane == 0) {
    inter[i * n + j] = count;
    inter[j * n + i] = count;
  }
}

__global__ void __launch_bounds__(kScanThreads)
scan(const int* __restrict__ inter, const int* __restrict__ area, int n, float nms_thr, unsigned char* __restrict__ keep) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int words = (n + 63) >> 6;
  unsigned long long* M = reinterpret_cast<unsigned long long*>(smem);      // [n][words]
  unsigned long long* remw = M + (size_t)n * words;                         // [words]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

  for (int i = wv; i < n; i += kScanThreads / 64) {
    const int ai = area[i];
    for (int w = 0; w < words; ++w) {
      if (i >= w * 64 + 63) {                  // no column of this word comes after row i
        if (lane == 0) M[i * words + w] = 0ull;
        continue;
      }
      const int j = w * 64 + lane;
      bool sup = false;
      if (j > i && j < n) {
        const int it = inter[i * n + j], un = ai + area[j] - it;
        sup = __fdiv_rn(__fadd_rn((float)it, 1e-6f), __fadd_rn((float)un, 1e-6f)) > nms_thr;
      }
      const unsigned long long word = __ballot(sup);
      if (lane == 0) M[i * words + w] = word;
    }
  }
  __syncthreads();

  if (wv == 0) {
    unsigned long long removed = 0ull;
    for (int w = 0; w < words; ++w) {
      unsigned long long cur = shfl64(removed, w);
      const int nb = min(64, n - w * 64);
      const unsigned long long* __restrict__ rows = M + (size_t)w * 64 * words;
      unsigned long long next = lane < words ? rows[lane] : 0ull;
      for (int bit = 0; bit < nb; ++bit) {
        const unsigned long long row = next;
        if (bit + 1 < nb) next = lane < words ? rows[(bit + 1) * words + lane] : 0ull;
        if (!((cur >> bit) & 1ull)) {          // wave-uniform: mask 64 w + bit is kept
          removed |= row;
          cur |= shfl64(row, w);
        }
      }
    }
    if (lane < words) remw[lane] = removed;
  }
  __syncthreads();
  if (tid < n) keep[tid] = ((remw[tid >> 6] >> lane) & 1ull) ? 0 : 1;
}

}  // namespace maskpost

extern "C" {

static const char* g_maskpost_last = "";

const char* maskpost_hip_last_kernel(void) { return g_maskpost_last; }

int maskpost_binarize_hip_f32(const float* logits, const long long* rows, int Q, int h, int w, int n, int stride, int crop_h,
                              int crop_w, int out_h, int out_w, float thres, unsigned char* out, void* stream) {
  using namespace maskpost;
  if (Q < 0 || h <= 0 || w <= 0 || n < 0 || crop_h < 1 || crop_w < 1 || out_h < 1 || out_w < 1)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "maskpost_binarize: bad dimensions");
  if (stride != 1 && stride != 2 && stride != 4 && stride != 8)
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "maskpost_binarize: stride must be 1, 2, 4 or 8");
  if (!(thres > 0.f && thres < 1.f)) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "maskpost_binarize: thres must lie in (0, 1)");
  if (w > kMaxW) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "maskpost_binarize: at most 8192 logits per row");
  if (crop_h > (long long)h * stride || crop_w > (long long)w * stride)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "maskpost_binarize: crop beyond the upsampled plane");
  constexpr long long kExtent = 1ll << 24;     // every index is exact as a float
  const int band = std::min(std::min(std::max(kBlendFloats / w, 1), kMaxBand), out_h);
  const long long xtiles = msda::ceil_div(out_w, kTileW), ybands = msda::ceil_div(out_h, band);
  if ((long long)Q * h * w >= (1ll << 31) || (long long)n * out_h * out_w >= (1ll << 31) || (long long)h * stride > kExtent ||
      (long long)w * stride > kExtent || out_h > kExtent || out_w > kExtent || xtiles * ybands * n >= (1ll << 31))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "maskpost_binarize: problem too large");
  if (n == 0) return 0;
  if (!logits || !rows || !out) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "maskpost_binarize: null pointer argument");
  const int tile_cap = msda::round_up(std::min(out_w, kTileW), 4);
  const size_t lds = (size_t)band * w * 4 + (size_t)tile_cap * 8;
  hipLaunchKernelGGL(binarize, dim3((unsigned)(xtiles * ybands * n)), dim3(kThreads), lds, (hipStream_t)stream, logits, rows, Q, h, w,
                     1.f / (float)stride, crop_h, crop_w, out_h, out_w, (float)crop_h / (float)out_h, (float)crop_w / (float)out_w,
                     thres, band, tile_cap, (int)xtiles, (int)ybands, out);
  if (const int e = msda::launch_status()) return e;
  g_maskpost_last = "maskpost_binarize";
  return 0;
}

int maskpost_pack_hip_f32(const float* logits, const long long* rows, int Q, int h, int w, int n, unsigned* bits, int* area,
                          void* stream) {
  using namespace maskpost;
  if (Q < 0 || h <= 0 || w <= 0 || n < 0) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "maskpost_pack: bad dimensions");
  const long long hw = (long long)h * w, words = msda::ceil_div(hw, 32ll);
  if (Q * hw >= (1ll << 31) || n * words >= (1ll << 31) || hw > (1ll << 30))
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "maskpost_pack: problem too large");
  if (n == 0) return 0;
  if (!logits || !rows || !bits || !area) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "maskpost_pack: null pointer argument");
  hipLaunchKernelGGL(pack, dim3((unsigned)n), dim3(kPackThreads), 0, (hipStream_t)stream, logits, rows, Q, (int)hw, (int)words, bits,
                     area);
  if (const int e = msda::launch_status()) return e;
  g_maskpost_last = "maskpost_pack";
  return 0;
}

int maskpost_nms_hip_u32(const unsigned* bits, const int* area, int n, int words, float nms_thr, int* inter, unsigned char* keep,
                     void* stream) {
  using namespace maskpost;
  static std::atomic<uint64_t> lds_opted_in{0};
  if (n < 0 || words <= 0) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "maskpost_nms: bad dimensions");
  if (n > kMaxN) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "maskpost_nms: at most 1024 masks");
  if ((long long)n * words >= (1ll << 31) || words > (1 << 26)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "maskpost_nms: problem too large");
  if (n == 0) return 0;
  if (!bits || !area || !inter || !keep) return msda::set_error(DYNMASK_ERR_NULL_POINTER, "maskpost_nms: null pointer argument");
  if (const int rc = msda::ensure_dynamic_lds(reinterpret_cast<const void*>(scan), kScanLdsMax, lds_opted_in))
    return msda::set_error(rc, "maskpost_nms: cannot reserve the kernel's LDS");
  hipLaunchKernelGGL(pairs, dim3((unsigned)msda::ceil_div(n, kThreads / 64), (unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, bits,
                     n, words, inter);
  const int words64 = msda::ceil_div(n, 64);
  hipLaunchKernelGGL(scan, dim3(1), dim3(kScanThreads), (size_t)(n * words64 + words64) * 8, (hipStream_t)stream, inter, area, n,
                     nms_thr, keep);
  if (const int e = msda::launch_status()) return e;
  g_maskpost_last = "maskpost_nms";
  return 0;
}

}  // extern "C"
