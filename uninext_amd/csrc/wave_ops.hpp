// Wave-level (wave64) butterfly reductions and shuffles of the kernels: every lane ends with the result; and the workgroup sum
// of doubles built on them.  Internal, device only.
// A namespace of its own: the sources under experiments/ keep a wave_max of theirs in namespace msda.
#pragma once

#include <hip/hip_runtime.h>

namespace wave_ops {

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// (value, index) reductions: the smallest / largest value, lowest index among equals
__device__ __forceinline__ void wave_argmin(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// lane `src`'s 64-bit value
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
  const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// Sum of K doubles per thread over a workgroup of WAVES waves; the result is valid on thread 0.  Fixed order: butterfly, then
// wave 0 .. WAVES - 1.
template <int K, int WAVES>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*red)[K]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wv][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s = red[0][k];
      for (int w = 1; w < WAVES; ++w) s += red[w][k];
      v[k] = s;
    }
  }
}

}  // namespace wave_ops

namespace msda {
using wave_ops::wave_sum;      // (msda_common.hpp had it; the MSDA kernels call it unqualified)
}
