// Detection post-processing: per-class scores of every decoder query, and class-aware NMS of an image's queries -- see
// include/dynmask_hip.h (detpost_scores_hip_f32, detpost_nms_hip_f32).
//
//   scores   one wave per (image, query) row, four rows per workgroup.  The row's T token logits are staged in LDS once; lane l
//            takes classes l, l + 64, ...: the sum of the class's tokens in list order, divided by their number (0.0 for a class
//            without tokens), the sigmoid, the optional sqrt(. * sigmoid(iou)), the threshold.  The row's maximum (first index
//            on ties) and its count of entries above the threshold are butterfly reductions over the wave.
//   nms      one workgroup of 16 waves per image, thread t owns query t.  Boxes become xyxy (plus the class offset of the
//            "coordinate trick" in mode 0), every thread counts the queries that precede its own (higher score, or equal score
//            and lower index) and moves its box to that rank.  The waves then fill the suppression matrix in rank order: a wave
//            keeps the 64 boxes of a column word in registers, reads one row box as an LDS broadcast and gets the word from one
//            ballot.  Wave 0 walks the ranks and ORs the rows of the boxes it keeps into the removed-mask (one 64-bit word per
//            lane), and all threads compact the kept ranks with popcounts.
//
// The box arithmetic is written with the __f*_rn intrinsics and the file is compiled without contraction: every operation
// rounds as one IEEE fp32 operation, as the same expression does on the CPU, so the kept indices can be compared exactly.  No
// atomics, fixed orders: bitwise repeatable.
#pragma clang fp contract(off)
#include "../../include/dynmask_hip.h"

#include <math.h>
#include <stdint.h>

#include <atomic>

#include "launch_glue.hpp"
#include "msda_common.hpp"

namespace detpost {

using msda::f32x4;
using msda::sigmoidf;
using wave_ops::shfl64;

constexpr int kScoreThreads = 256;
constexpr int kScoreRows = kScoreThreads / 64;
constexpr int kMaxT = DETPOST_HIP_MAX_TOKENS;
constexpr int kMaxC = DETPOST_HIP_MAX_CLASSES;
constexpr int kMaxQ = DETPOST_HIP_MAX_QUERIES;
constexpr int kNmsThreads = 1024;
constexpr int kMaxWords = kMaxQ / 64;
// dynamic LDS of the NMS kernel at Q = 1024: rank-ordered boxes (16 B each), their classes and query indices (4 B each) and
// the 1024 x 16 matrix of 64-bit words; the 192 B of static LDS next to it keep the total under the 160 KB of a CU
constexpr int kNmsLdsMax = kMaxQ * (16 + 4 + 4) + kMaxQ * kMaxWords * 8;
static_assert(kNmsLdsMax + 256 <= 160 * 1024, "one workgroup per CU");
static_assert(kMaxQ <= kNmsThreads && kMaxWords <= 64, "a thread per query, a lane per mask word");

__global__ void __launch_bounds__(kScoreThreads)
scores(const float* __restrict__ logits, const float* __restrict__ iou_logits, const int* __restrict__ cls_ptr,
       const int* __restrict__ tok_idx, int nnz, float score_thres, int rows, int C, int T, float* __restrict__ prob,
       float* __restrict__ row_max, int* __restrict__ row_arg, int* __restrict__ row_valid) {
  __shared__ float Ls[kScoreRows][kMaxT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = blockIdx.x * kScoreRows + wv;
  if (row >= rows) return;                     // wave-uniform; no barrier below: a wave only reads what it staged itself
  const float* __restrict__ src = logits + (long long)row * T;
  for (int t = lane; t < T; t += 64) Ls[wv][t] = src[t];
  const bool with_iou = iou_logits != nullptr;
  const float siou = with_iou ? sigmoidf(iou_logits[row]) : 1.f;
  float best = -__builtin_inff();
  int arg = 0x7fffffff, valid = 0;
  for (int c = lane; c < C; c += 64) {
    const int lo = min(max(cls_ptr[c], 0), nnz), hi = min(max(cls_ptr[c + 1], lo), nnz);
    float mean = 0.f;
    if (hi > lo) {
      float sum = 0.f;
      for (int k = lo; k < hi; ++k) {
        const int t = tok_idx[k];
        sum += (unsigned)t < (unsigned)T ? Ls[wv][t] : 0.f;
      }
      mean = __fdiv_rn(sum, (float)(hi - lo));
    }
    float p = sigmoidf(mean);
    if (with_iou) p = __fsqrt_rn(__fmul_rn(p, siou));
    if (score_thres > 0.f) {
      if (p > score_thres) ++valid;
      else p = -1.f;
    }
    prob[(long long)row * C + c] = p;
    if (p > best) best = p, arg = c;           // c ascends on the lane: the first index of the lane's maximum
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {           // (written out: wave_ops::wave_argmax + wave_sum change this kernel's assembly)
    const float ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    valid += __shfl_xor(valid, o, 64);
    if (ob > best || (ob == best && oa < arg)) best = ob, arg = oa;
  }
  if (lane == 0) {
    row_max[row] = best;
    row_arg[row] = arg == 0x7fffffff ? 0 : arg;          // a row of NaNs: index 0
    row_valid[row] = valid;
  }
}

__global__ void __launch_bounds__(kNmsThreads)
nms(const float* __restrict__ boxes, const float* __restrict__ row_max, const int* __restrict__ row_arg, float iou_threshold,
    int per_class, int Q, int* __restrict__ keep, int* __restrict__ n_keep, unsigned char* __restrict__ kept_mask) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red[kNmsThreads / 64];
  __shared__ unsigned long long remw[kMaxWords];
  const int words = (Q + 63) >> 6, Qp = words * 64;
  f32x4* sbox = reinterpret_cast<f32x4*>(smem);                         // [Qp] xyxy in rank order
  int* scls = reinterpret_cast<int*>(smem + (size_t)Qp * 16);           // [Qp]
  int* sidx = scls + Qp;                                                // [Qp] query of the rank
  unsigned long long* M = reinterpret_cast<unsigned long long*>(smem + (size_t)Qp * 24);   // [Q][words]
  float* ssc = reinterpret_cast<float*>(M);                             // [Q] scores by query, until the matrix is written
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long base = (long long)blockIdx.x * Q;
  const bool mine = tid < Q;

  f32x4 bx = {0.f, 0.f, 0.f, 0.f};
  float sc = 0.f;
  int cls = 0;
  if (mine) {
    const f32x4 c = *reinterpret_cast<const f32x4*>(boxes + (base + tid) * 4);
    const float hw = __fmul_rn(0.5f, c[2]), hh = __fmul_rn(0.5f, c[3]);
    bx[0] = __fsub_rn(c[0], hw);
    bx[1] = __fsub_rn(c[1], hh);
    bx[2] = __fadd_rn(c[0], hw);
    bx[3] = __fadd_rn(c[1], hh);
    sc = row_max[base + tid];
    if (sc != sc) sc = __builtin_inff();       // a NaN score sorts first; the ranks stay a permutation
    cls = row_arg[base + tid];
    ssc[tid] = sc;
  }
  if (!per_class) {                            // offset every class into a range of its own
    float m = mine ? fmaxf(fmaxf(bx[0], bx[1]), fmaxf(bx[2], bx[3])) : -__builtin_inff();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));   // (written out: wave_ops::wave_max changes this kernel's assembly)
    if (lane == 0) red[wv] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < kNmsThreads / 64; ++w) m = fmaxf(m, red[w]);
    const float off = __fmul_rn((float)cls, __fadd_rn(m, 1.f));
#pragma unroll
    for (int e = 0; e < 4; ++e) bx[e] = __fadd_rn(bx[e], off);
  }
  __syncthreads();                             // ssc complete
  int rank = 0;
  if (mine) {
    for (int j = 0; j < Q; ++j) {
      const float sj = ssc[j];
      rank += (sj > sc || (sj == sc && j < tid)) ? 1 : 0;
    }
  }
  __syncthreads();                             // every thread has read ssc: the region becomes the matrix
  if (mine) {
    sbox[rank] = bx;
    scls[rank] = cls;
    sidx[rank] = tid;
  } else if (tid < Qp) {                       // ranks past the end: never a row, masked out as a column
    sbox[tid] = f32x4{0.f, 0.f, 0.f, 0.f};
    scls[tid] = -1;
    sidx[tid] = -1;
  }
  __syncthreads();

  for (int w = 0; w < words; ++w) {
    const int j = w * 64 + lane;
    const f32x4 bj = sbox[j];
    const int cj = scls[j];
    const float aj = __fmul_rn(__fsub_rn(bj[2], bj[0]), __fsub_rn(bj[3], bj[1]));
    for (int i = wv; i < Q; i += kNmsThreads / 64) {
      if (i >= w * 64 + 63) {                  // no column of this word comes after row i
        if (lane == 0) M[i * words + w] = 0ull;
        continue;
      }
      const f32x4 bi = sbox[i];
      const float ai = __fmul_rn(__fsub_rn(bi[2], bi[0]), __fsub_rn(bi[3], bi[1]));
      const float iw = fmaxf(__fsub_rn(fminf(bi[2], bj[2]), fmaxf(bi[0], bj[0])), 0.f);
      const float ih = fmaxf(__fsub_rn(fminf(bi[3], bj[3]), fmaxf(bi[1], bj[1])), 0.f);
      const float inter = __fmul_rn(iw, ih);
      bool sup = false;
      if (j > i && j < Q && (!per_class || cj == scls[i]) && (inter > 0.f || iou_threshold < 0.f))
        sup = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ai, aj), inter)) > iou_threshold;     // 0 / 0: NaN, not suppressed
      const unsigned long long word = __ballot(sup);
      if (lane == 0) M[i * words + w] = word;
    }
  }
  __syncthreads();

  if (wv == 0) {
    unsigned long long removed = 0ull;
    for (int w = 0; w < words; ++w) {
      unsigned long long cur = shfl64(removed, w);
      const int nb = min(64, Q - w * 64);
      const unsigned long long* __restrict__ rows = M + (size_t)w * 64 * words;
      unsigned long long next = lane < words ? rows[lane] : 0ull;
      for (int bit = 0; bit < nb; ++bit) {
        const unsigned long long row = next;
        if (bit + 1 < nb) next = lane < words ? rows[(bit + 1) * words + lane] : 0ull;
        if (!((cur >> bit) & 1ull)) {          // wave-uniform: rank 64 w + bit is kept
          removed |= row;
          cur |= shfl64(row, w);
        }
      }
    }
    if (lane < words) remw[lane] = removed;
  }
  __syncthreads();

  // a bit of the removed-mask is final once its rank has been visited: kept = not removed
  int total = 0, before = 0;
  for (int w = 0; w < words; ++w) {
    const unsigned long long live = w == words - 1 && (Q & 63) ? (1ull << (Q & 63)) - 1ull : ~0ull;
    const unsigned long long k = ~remw[w] & live;
    total += __popcll(k);
    if (w < (tid >> 6)) before += __popcll(k);
    else if (w == (tid >> 6)) before += __popcll(k & ((1ull << lane) - 1ull));
  }
  if (mine) {
    const bool kept = !((remw[tid >> 6] >> lane) & 1ull);
    const int q = sidx[tid];
    kept_mask[base + q] = kept ? 1 : 0;
    if (kept) keep[base + before] = q;
    if (tid >= total) keep[base + tid] = -1;
  }
  if (tid == 0) n_keep[blockIdx.x] = total;
}

}  // namespace detpost

extern "C" {

static const char* g_detpost_last = "";

const char* detpost_hip_last_kernel(void) { return g_detpost_last; }

int detpost_scores_hip_f32(const float* logits, const float* iou_logits, const int* cls_ptr, const int* tok_idx, int nnz,
                           float score_thres, int batch, int Q, int C, int T, float* prob, float* row_max, int* row_arg,
                           int* row_valid, void* stream) {
  if (batch < 0 || Q < 0 || C <= 0 || T <= 0 || nnz < 0) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "detpost_scores: bad dimensions");
  if (C > detpost::kMaxC || T > detpost::kMaxT)
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "detpost_scores: at most 4096 classes and 256 tokens");
  const long long rows = (long long)batch * Q;
  if (rows * C >= (1ll << 31) || rows * T >= (1ll << 31)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "detpost_scores: problem too large");
  if (rows == 0) return 0;
  if (!logits || !cls_ptr || (nnz > 0 && !tok_idx) || !prob || !row_max || !row_arg || !row_valid)
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "detpost_scores: null pointer argument");
  const dim3 grid((unsigned)((rows + detpost::kScoreRows - 1) / detpost::kScoreRows)), block(detpost::kScoreThreads);
  hipLaunchKernelGGL(detpost::scores, grid, block, 0, (hipStream_t)stream, logits, iou_logits, cls_ptr, tok_idx, nnz, score_thres,
                     (int)rows, C, T, prob, row_max, row_arg, row_valid);
  if (const int e = msda::launch_status()) return e;
  g_detpost_last = iou_logits ? "detpost_scores<iou>" : "detpost_scores";
  return 0;
}

int detpost_nms_hip_f32(const float* boxes, const float* row_max, const int* row_arg, float iou_threshold, int per_class,
                        int batch, int Q, int* keep, int* n_keep, unsigned char* kept_mask, void* stream) {
  static std::atomic<uint64_t> lds_opted_in{0};
  if (batch < 0 || Q < 0 || (per_class != 0 && per_class != 1)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "detpost_nms: bad dimensions");
  if (Q > detpost::kMaxQ) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "detpost_nms: at most 1024 queries per image");
  if (batch == 0) return 0;
  if (!n_keep || (Q > 0 && (!boxes || !row_max || !row_arg || !keep || !kept_mask)))
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "detpost_nms: null pointer argument");
  if (!msda::aligned16({boxes})) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "detpost_nms: boxes must be 16-byte aligned");
  if (const int rc = msda::ensure_dynamic_lds(reinterpret_cast<const void*>(detpost::nms), detpost::kNmsLdsMax, lds_opted_in))
    return msda::set_error(rc, "detpost_nms: cannot reserve the kernel's LDS");
  const int words = msda::ceil_div(Q, 64);
  const size_t lds = (size_t)words * 64 * 24 + (size_t)Q * words * 8;
  hipLaunchKernelGGL(detpost::nms, dim3((unsigned)batch), dim3(detpost::kNmsThreads), lds, (hipStream_t)stream, boxes, row_max,
                     row_arg, iou_threshold, per_class, Q, keep, n_keep, kept_mask);
  if (const int e = msda::launch_status()) return e;
  g_detpost_last = per_class ? "detpost_nms<per_class>" : "detpost_nms<offset>";
  return 0;
}

}  // extern "C"
