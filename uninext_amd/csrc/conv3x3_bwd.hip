// Backward of the exact-fp32 3x3 convolution + ReLU of conv3x3.hip (stride 1, zero padding 1) -- see include/conv3x3_hip.h.
//
//   g[b, n, y, x]       = grad_out[b, n, y, x] if out[b, n, y, x] > 0 else 0          (relu != 0; else g = grad_out)
//   grad_bias[n]        = sum_{b, y, x} g[b, n, y, x]
//   grad_in[b, c, y, x] = sum_{n, ky, kx} g[b, n, y + ky - 1, x + kx - 1] * W[n, c, 2 - ky, 2 - kx]
//   grad_w[n, c, ky, kx] = sum_{b, y, x} g[b, n, y, x] * in[b, c, y + ky - 1, x + kx - 1]
//
// Three pieces:
//   * relu_bias_kernel: one pass over grad_out / out that writes g into a workspace buffer whose channel count is padded up to a
//     multiple of 16 (padding zero-filled) and the per-image partial sums of the bias gradient (fixed thread order, fixed tree);
//   * grad-input: grad_in is the 3x3 convolution of g with the transposed, flipped weights -- pack_weight_dgrad_kernel writes them
//     straight into the layout of conv3x3_exact (conv3x3.hip), and conv3x3_hip_packed_exact_f32 runs it unchanged (no bias, no ReLU);
//   * grad-weight, conv3x3_wgrad: a GEMM with M = cout, N = 9 cin, K = B H W pixels on v_mfma_f32_32x32x2_f32.  A workgroup owns
//     64 output x 64 input channels x the nine taps and a fixed range of 4 x 16 pixel tiles (split-K, a function of the shape
//     only); per tile it stages the g tile [64 n][64 pixels] and the 6 x 18 halo of the 64 input channels in LDS and serves all
//     nine taps from the one halo with immediate offsets.  A wave keeps one 32 x 32 accumulator per tap (9 x 16 registers).  The
//     partial sums of the splits go to the workspace and wgrad_reduce_kernel adds them in split order: no float atomics, every
//     output is a fixed chain of fp32 operations -- bitwise repeatable across runs, streams and processes.
#include "../../include/conv3x3_hip.h"

#include "launch_glue.hpp"
#include "mfma_frag.hpp"
#include "msda_common.hpp"

namespace conv3x3_bwd {

using namespace mfma_frag;
using msda::align256;
using msda::f32x4;

constexpr int kThreads = 256;
constexpr int kChunk = 16;                 // channel granularity of the exact forward kernel
constexpr int kTH = 4, kTW = 16;           // pixel tile of the grad-weight kernel
constexpr int kTilePx = kTH * kTW;         // 64
constexpr int kBN = 64, kBC = 64;          // output / input channels of a grad-weight workgroup
constexpr int kGPitch = kTilePx + 4;       // floats per g row in LDS: a ds_read_b128 of 16 lanes (16 channels) covers all 64 banks
constexpr int kXRows = kTH + 2, kXCols = kTW + 2;
constexpr int kXPlane = kXRows * kXCols + 1;   // 109 floats per input channel: odd, so the 32 channels of a ds_read_b32 hit 32 banks
constexpr int kTargetGroups = 512;         // grad-weight workgroups a launch aims at (2 per CU of the MI355X)
constexpr int kMaxSplits = 256;

inline int pad16(int c) { return (c + kChunk - 1) / kChunk * kChunk; }

// Split-K of the grad-weight kernel: the number of pixel-tile ranges depends on the shape only
inline int wgrad_splits(int batch, int cin, int height, int width, int cout) {
  const long long tiles = (long long)batch * ((height + kTH - 1) / kTH) * ((width + kTW - 1) / kTW);
  const long long groups = (long long)((cout + kBN - 1) / kBN) * ((cin + kBC - 1) / kBC);
  long long s = (kTargetGroups + groups - 1) / groups;
  if (s > kMaxSplits) s = kMaxSplits;
  if (s > tiles) s = tiles;
  return s < 1 ? 1 : (int)s;
}

struct Layout {   // byte offsets of the workspace parts
  size_t g, wparts, bparts, total;
  int splits;
};

inline Layout layout(int batch, int cin, int height, int width, int cout) {
  Layout l;
  l.splits = wgrad_splits(batch, cin, height, width, cout);
  l.g = 0;
  l.wparts = align256((size_t)batch * pad16(cout) * height * width * sizeof(float));
  l.bparts = l.wparts + align256((size_t)l.splits * cout * cin * 9 * sizeof(float));
  l.total = l.bparts + align256((size_t)batch * cout * sizeof(float));
  return l;
}

// grid (cout_p, batch): g of one (image, channel) plane and its sum
__global__ void __launch_bounds__(kThreads)
relu_bias_kernel(const float* __restrict__ out, const float* __restrict__ grad_out, int relu, int cout, int cout_p, int HW,
                 float* __restrict__ g, float* __restrict__ bparts) {
  __shared__ float red[kThreads];
  const int n = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float* dst = g + ((int64_t)b * cout_p + n) * HW;
  if (n >= cout) {
    for (int p = tid; p < HW; p += kThreads) dst[p] = 0.f;
    return;
  }
  const int64_t src = ((int64_t)b * cout + n) * HW;
  float sum = 0.f;
  if ((HW & 3) == 0) {
    const f32x4* go4 = reinterpret_cast<const f32x4*>(grad_out + src);
    const f32x4* o4 = reinterpret_cast<const f32x4*>(out + src);
    f32x4* d4 = reinterpret_cast<f32x4*>(dst);
    for (int q = tid; q < HW / 4; q += kThreads) {
      f32x4 v = go4[q];
      if (relu) {
        const f32x4 o = o4[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = o[e] <= 0.f ? 0.f : v[e];
      }
      d4[q] = v;
      sum += (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int p = tid; p < HW; p += kThreads) {
      float v = grad_out[src + p];
      if (relu && out[src + p] <= 0.f) v = 0.f;
      dst[p] = v;
      sum += v;
    }
  }
  red[tid] = sum;
  __syncthreads();
#pragma unroll
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) bparts[(int64_t)b * cout + n] = red[0];
}

// W [cout, cin, 3, 3] -> the exact kernel's packed layout of W'[c, n, ky, kx] = W[n, c, 2 - ky, 2 - kx], a convolution with
// cin' = cout_p (cout rounded up to 16, zero weights for the padding) input and cin output channels:
// [cout_p / 16][9 taps][cin padded to 128][16], position 8 h + s of a chunk = channel 2 s + h (conv3x3.hip: pack_weight_exact_kernel)
__global__ void pack_weight_dgrad_kernel(const float* __restrict__ w, int cout, int cin, int cout_p, int cin_pad,
                                         float* __restrict__ packed) {
  const int64_t total = (int64_t)(cout_p / kChunk) * 9 * cin_pad * kChunk;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int pos = (int)(idx % kChunk);
    const int c = (int)((idx / kChunk) % cin_pad);
    const int tap = (int)((idx / kChunk / cin_pad) % 9);
    const int chunk = (int)(idx / kChunk / cin_pad / 9);
    const int n = chunk * kChunk + 2 * (pos & 7) + (pos >> 3);
    packed[idx] = (c < cin && n < cout) ? w[((int64_t)n * cin + c) * 9 + (8 - tap)] : 0.f;
  }
}

// grid (output-channel blocks x input-channel blocks, splits).  Wave (wn, wc) of the 2 x 2 owns output channels n0 + 32 wn ..,
// input channels c0 + 32 wc .. and nine accumulators, one per tap: accumulator register v of lane l is
// (output channel 8 (v / 4) + 4 (l / 32) + v % 4, input channel l % 32) -- g is the first MFMA operand.
// The reduction over a tile's pixels: a group of 8 columns of a tile row; in k-step s lanes 0-31 take column s, lanes 32-63 column 4 + s.
__global__ void __launch_bounds__(kThreads, 2)
conv3x3_wgrad(const float* __restrict__ in, const float* __restrict__ g, int B, int cin, int H, int W, int cout, int cout_p,
              int tiles_x, int tiles_per_image, int ntiles, int splits, float* __restrict__ wparts) {
  __shared__ __attribute__((aligned(16))) float Gs[kBN * kGPitch];
  __shared__ float Xs[kBC * kXPlane];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nblocks = (cout + kBN - 1) / kBN;
  const int n0 = (blockIdx.x % nblocks) * kBN, c0 = (blockIdx.x / nblocks) * kBC;
  const int split = blockIdx.y;
  const int t_begin = (int)((long long)ntiles * split / splits), t_end = (int)((long long)ntiles * (split + 1) / splits);
  const int HW = H * W;
  const int wn = wv >> 1, wc = wv & 1, r32 = lane & 31, half = lane >> 5;

  f32x16 acc[9];
  zero_acc(acc);

  const float* g_lane = Gs + (wn * 32 + r32) * kGPitch + 4 * half;
  const float* x_lane = Xs + (wc * 32 + r32) * kXPlane + 4 * half;

  for (int t = t_begin; t < t_end; ++t) {
    const int b = t / tiles_per_image, ti = t - b * tiles_per_image;
    const int ty0 = (ti / tiles_x) * kTH, tx0 = (ti % tiles_x) * kTW;
    __syncthreads();   // the previous tile's readers are done
    // g tile: items (channel, pixel), pixel fastest -- 16 per thread
#pragma unroll 4
    for (int i = 0; i < kBN * kTilePx / kThreads; ++i) {
      const int item = tid + i * kThreads;
      const int nl = item / kTilePx, p = item % kTilePx;
      const int n = n0 + nl, y = ty0 + p / kTW, x = tx0 + p % kTW;
      Gs[nl * kGPitch + p] = (n < cout_p && y < H && x < W) ? g[((int64_t)b * cout_p + n) * HW + y * W + x] : 0.f;
    }
    // input halo: items (channel, halo row, halo column), column fastest -- 27 per thread
#pragma unroll 3
    for (int i = 0; i < (kBC * kXRows * kXCols + kThreads - 1) / kThreads; ++i) {
      const int item = tid + i * kThreads;
      if (item < kBC * kXRows * kXCols) {
        const int cl = item / (kXRows * kXCols), r = item % (kXRows * kXCols);
        const int hr = r / kXCols, hc = r % kXCols;
        const int c = c0 + cl, y = ty0 - 1 + hr, x = tx0 - 1 + hc;
        const bool ok = c < cin && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        Xs[cl * kXPlane + hr * kXCols + hc] = ok ? in[((int64_t)b * cin + c) * HW + y * W + x] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kTH; ++r)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g_lane + r * kTW + 8 * j);
        float xv[9][4];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
          for (int s = 0; s < 4; ++s) xv[tap][s] = x_lane[(r + tap / 3) * kXCols + 8 * j + tap % 3 + s];
        // k-step outermost: consecutive MFMAs go to different accumulators
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[s], xv[tap][s], acc[tap], 0, 0, 0);
      }
  }

  // partial sums of this split: wparts [splits][cout][cin][9]
  const int c = c0 + wc * 32 + r32;
  if (c < cin) {
    float* dst = wparts + (int64_t)split * cout * cin * 9;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int n = n0 + wn * 32 + acc_row(v, half);
      if (n < cout) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) dst[((int64_t)n * cin + c) * 9 + tap] = acc[tap][v];
      }
    }
  }
}

// grad_weight = sum of the splits' partial sums in split order; grad_bias = sum of the images' partial sums in image order
__global__ void __launch_bounds__(kThreads)
wgrad_reduce_kernel(const float* __restrict__ wparts, int splits, int64_t wtotal, float* __restrict__ grad_weight,
                    const float* __restrict__ bparts, int batch, int cout, float* __restrict__ grad_bias) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < wtotal + cout; idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx < wtotal) {
      if (!grad_weight) continue;
      // eight loads in flight, then their sums in split order (a chain of dependent loads waits for memory at every split)
      float s = 0.f;
      int k = 0;
      for (; k + 8 <= splits; k += 8) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = wparts[(int64_t)(k + e) * wtotal + idx];
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[e];
      }
      for (; k < splits; ++k) s += wparts[(int64_t)k * wtotal + idx];
      grad_weight[idx] = s;
    } else if (grad_bias) {
      const int n = (int)(idx - wtotal);
      float s = 0.f;
      for (int b = 0; b < batch; ++b) s += bparts[(int64_t)b * cout + n];
      grad_bias[n] = s;
    }
  }
}

}  // namespace conv3x3_bwd

extern "C" {

size_t conv3x3_hip_packed_exact_dgrad_weight_bytes(int cout, int cin) {
  if (cout <= 0 || cin <= 0) return 0;
  return conv3x3_hip_packed_exact_weight_bytes(cin, conv3x3_bwd::pad16(cout));
}

int conv3x3_hip_pack_weight_exact_dgrad_f32(const float* weight, int cout, int cin, void* packed, void* stream) {
  if (cout <= 0 || cin <= 0) return msda::set_error(CONV3X3_ERR_BAD_DIMS, "conv3x3: bad dimensions");
  if (!weight || !packed) return msda::set_error(CONV3X3_ERR_NULL_POINTER, "conv3x3: null pointer argument");
  const int cin_pad = msda::round_up(cin, 128);   // the exact kernel's output-channel padding (gemm_core.hpp: padded128)
  hipLaunchKernelGGL(conv3x3_bwd::pack_weight_dgrad_kernel, dim3(512), dim3(256), 0, (hipStream_t)stream, weight, cout, cin,
                     conv3x3_bwd::pad16(cout), cin_pad, static_cast<float*>(packed));
  return msda::launch_status();
}

size_t conv3x3_hip_backward_workspace_bytes(int batch, int cin, int height, int width, int cout) {
  if (batch < 0 || cin <= 0 || height <= 0 || width <= 0 || cout <= 0) return 0;
  if (batch == 0) return 0;
  return conv3x3_bwd::layout(batch, cin, height, width, cout).total;
}

int conv3x3_hip_backward_exact_f32(const float* in, const void* packed_dgrad, const float* out, const float* grad_out, int batch,
                                   int cin, int height, int width, int cout, int relu, float* grad_in, float* grad_weight,
                                   float* grad_bias, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace conv3x3_bwd;
  if (batch < 0 || cin <= 0 || height <= 0 || width <= 0 || cout <= 0)
    return msda::set_error(CONV3X3_ERR_BAD_DIMS, "conv3x3 backward: bad dimensions");
  hipStream_t st = (hipStream_t)stream;
  if (batch == 0) {   // the gradients of a sum over no pixels
    if (grad_weight && hipMemsetAsync(grad_weight, 0, (size_t)cout * cin * 9 * sizeof(float), st) != hipSuccess)
      return msda::launch_status();
    if (grad_bias && hipMemsetAsync(grad_bias, 0, (size_t)cout * sizeof(float), st) != hipSuccess)
      return msda::launch_status();
    return 0;
  }
  const int cout_p = pad16(cout);
  const long long HW = (long long)height * width;
  const int tiles_x = msda::ceil_div(width, kTW), tiles_y = msda::ceil_div(height, kTH);
  const long long ntiles = (long long)batch * tiles_x * tiles_y;
  if ((long long)batch * cout_p * HW >= (1ll << 31) || (long long)batch * cin * HW >= (1ll << 31) || ntiles >= (1ll << 31)
      || (long long)cout * cin * 9 >= (1ll << 31))
    return msda::set_error(CONV3X3_ERR_BAD_DIMS, "conv3x3 backward: problem too large");
  if (!grad_in && !grad_weight && !grad_bias) return 0;
  if (!grad_out || (relu && !out) || !workspace || (grad_in && !packed_dgrad) || (grad_weight && !in))
    return msda::set_error(CONV3X3_ERR_NULL_POINTER, "conv3x3 backward: null pointer argument");
  const Layout l = layout(batch, cin, height, width, cout);
  if (workspace_bytes < l.total)
    return msda::set_error(CONV3X3_ERR_BAD_DIMS, "conv3x3 backward: workspace smaller than conv3x3_hip_backward_workspace_bytes");
  char* ws = static_cast<char*>(workspace);
  float* g = reinterpret_cast<float*>(ws + l.g);
  float* wparts = reinterpret_cast<float*>(ws + l.wparts);
  float* bparts = reinterpret_cast<float*>(ws + l.bparts);

  hipLaunchKernelGGL(relu_bias_kernel, dim3((unsigned)cout_p, (unsigned)batch), dim3(kThreads), 0, st, out, grad_out, relu, cout,
                     cout_p, (int)HW, g, bparts);
  int rc = msda::launch_status();
  if (rc) return rc;
  if (grad_in) {
    rc = conv3x3_hip_packed_exact_f32(g, packed_dgrad, nullptr, batch, cout_p, height, width, cin, 0, grad_in, stream);
    if (rc) return rc;
  }
  if (grad_weight) {
    const int groups = msda::ceil_div(cout, kBN) * msda::ceil_div(cin, kBC);
    hipLaunchKernelGGL(conv3x3_wgrad, dim3((unsigned)groups, (unsigned)l.splits), dim3(kThreads), 0, st, in, g, batch, cin, height,
                       width, cout, cout_p, tiles_x, tiles_x * tiles_y, (int)ntiles, l.splits, wparts);
    rc = msda::launch_status();
    if (rc) return rc;
  }
  if (grad_weight || grad_bias) {
    const int64_t wtotal = (int64_t)cout * cin * 9;
    long long blocks = (wtotal + cout + kThreads - 1) / kThreads;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, wparts, l.splits, wtotal, grad_weight,
                       bparts, batch, cout, grad_bias);
    rc = msda::launch_status();
  }
  return rc;
}

}  // extern "C"
