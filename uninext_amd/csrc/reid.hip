// ota_reid_select_hip / ota_reid_scores_hip_f32 / ota_reid_loss_hip_f32 / ota_reid_loss_bwd_hip_f32 (include/ota_hip.h): the re-ID contrastive
// training of the video configs on the device -- projects/UNINEXT/uninext/models/pos_neg_select.py (get_pos_idx :99-153,
// dynamic_k_matching :187-226, select_pos_neg :15-94) and loss_reid (deformable_detr.py:529-565).  gfx950.
//
// Selection: the cost matrix is ota_cost_hip_f32's; the assignment is dynamic_k.hpp's, the one ota.hip runs, with 10 and then 100
// candidates, a per-target `valid` byte (an invalid target is an absent column) and two runs over ONE cost matrix -- the second run
// sees the + 100000 rows the first run's repair loop left (the reference passes the same tensor twice).  Its outputs are
// integers, so float contraction is off for the whole file and the scores' FMA chains are written out as fmaf.
//
// Scores and loss: plain FMA at these sizes ([900, 256] x [256, ~10] per image).  No float atomics: every sum has one owner and a
// fixed order, so every kernel is bitwise repeatable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ota_hip.h"
#include "launch_glue.hpp"

#pragma clang fp contract(off)

#include "dynamic_k.hpp"

namespace reid {
namespace {

using msda::BatchOffsets;
using msda::dynamic_k;
using msda::kMaxGt;

constexpr float kBgPenalty = 10000.0f;                              // pos_neg_select.py:122
constexpr int kPosCandidates = 10, kNegCandidates = 100;            // pos_neg_select.py:130-131
constexpr float kNormEps = 1e-12f;                                  // F.normalize's eps

constexpr int kST = 1024, kSW = kST / 64;

__global__ void __launch_bounds__(kST)
reid_select_kernel(float* __restrict__ cost, const float* __restrict__ iou, const uint8_t* __restrict__ flags,
                   const uint8_t* __restrict__ valid, const long long* __restrict__ key_index, BatchOffsets go, int Q, int Qk,
                   int max_rounds, uint8_t* __restrict__ mpos, uint8_t* __restrict__ mneg, int32_t* __restrict__ counts,
                   int32_t* __restrict__ status) {
  __shared__ uint8_t s_unmatched[kMaxGt];
  __shared__ int s_count[2];
  const int b = blockIdx.x;
  const int g0 = go.off[b], G = go.off[b + 1] - g0;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (G <= 0) {
    if (tid == 0) status[b] = 0;
    return;
  }
  float* const C = cost + (int64_t)Q * g0;
  const float* const I = iou + (int64_t)Q * g0;
  const uint8_t* const F = flags + (int64_t)Q * g0;
  const uint8_t* const V = valid + g0;
  uint8_t* const Mp = mpos + (int64_t)Q * g0;
  uint8_t* const Mn = mneg + (int64_t)Q * g0;

  int nvalid = 0, bad_index = 0;
  for (int g = 0; g < G; ++g) {
    if (!V[g]) continue;
    ++nvalid;
    long long k = key_index[g0 + g];
    if (k < 0) k += Qk;
    if (k < 0 || k >= Qk) bad_index = 8;
  }
  if (nvalid == 0) {                              // (uniform over the workgroup) no items: zeroed matrices, no counts
    for (int64_t e = tid; e < (int64_t)Q * G; e += kST) { Mp[e] = 0; Mn[e] = 0; }
    for (int g = tid; g < G; g += kST) { counts[2 * (g0 + g)] = -1; counts[2 * (g0 + g) + 1] = -1; }
    if (tid == 0) status[b] = 0;
    return;
  }

  // ---- the background penalty, ONCE (pos_neg_select.py:122; fg_mask: inside ANY existing box or centre square) ----------------
  int bad = 0;
  for (int q = tid; q < Q; q += kST) {
    bool fg = false;
    for (int g = 0; g < G; ++g) {
      if (!V[g]) continue;
      const uint8_t f = F[(int64_t)q * G + g];
      fg = fg || (f & 1) != 0;
      bad |= f & 2;
    }
    if (!fg)
      for (int g = 0; g < G; ++g) C[(int64_t)q * G + g] = C[(int64_t)q * G + g] + kBgPenalty;
  }
  const int degenerate = __syncthreads_or(bad) ? 4 : 0;

  int st = dynamic_k<true, kST>(C, I, Mp, V, Q, G, min(Q, kPosCandidates), max_rounds, s_unmatched, s_count);
  st |= dynamic_k<true, kST>(C, I, Mn, V, Q, G, min(Q, kNegCandidates), max_rounds, s_unmatched, s_count);   // on the cost as the first run left it

  for (int g = wv; g < G; g += kSW) {
    int np = 0, nm = 0;
    if (V[g])
      for (int q = lane; q < Q; q += 64) { np += Mp[(int64_t)q * G + g]; nm += Mn[(int64_t)q * G + g]; }
    np = wave_ops::wave_sum(np);
    nm = wave_ops::wave_sum(nm);
    if (lane == 0) {
      counts[2 * (g0 + g)] = V[g] ? np : -1;
      counts[2 * (g0 + g) + 1] = V[g] ? Q - nm : -1;
    }
  }
  if (tid == 0) status[b] = st | degenerate | bad_index;
}

// the key row of a target: Python's negative indexing, clamped into the tensor (ota_reid_select_hip reports an index outside it)
__device__ __forceinline__ int key_row(const long long* __restrict__ key_index, int target, int n_targets, int Qk) {
  long long k = key_index[min(max(target, 0), n_targets - 1)];
  if (k < 0) k += Qk;
  return (int)(k < 0 ? 0 : (k >= Qk ? Qk - 1 : k));
}

// ---- scores ---------------------------------------------------------------------------------------------------------------------
constexpr int kTQ = 16;                           // reference rows per tile: staged in LDS once, used by every target of the image
constexpr int kScT = 256;

__global__ void __launch_bounds__(kScT)
reid_scores_kernel(const float* __restrict__ ref, const float* __restrict__ key, const long long* __restrict__ key_index,
                   const uint8_t* __restrict__ valid, BatchOffsets go, int Q, int Qk, int C, float* __restrict__ dot,
                   float* __restrict__ cosv, float* __restrict__ ref_norm, float* __restrict__ key_norm) {
  __shared__ float s_ref[kTQ * (REID_HIP_MAX_DIM + 1)];      // row stride C + 1: the 16 rows of a wave fall into 16 banks
  const int b = blockIdx.y, q0 = blockIdx.x * kTQ, tid = threadIdx.x;
  const int g0 = go.off[b], G = go.off[b + 1] - g0;
  if (G <= 0) return;
  const int rows = min(kTQ, Q - q0);
  for (int e = tid; e < rows * C; e += kScT) {
    const int r = e / C, c = e - r * C;
    s_ref[r * (C + 1) + c] = ref[((int64_t)b * Q + q0 + r) * C + c];
  }
  __syncthreads();
  int first_valid = -1;
  for (int g = G - 1; g >= 0; --g)
    if (valid[g0 + g]) first_valid = g;
  for (int item = tid; item < kTQ * G; item += kScT) {
    const int ql = item % kTQ, gl = item / kTQ;
    if (ql >= rows) continue;
    const int q = q0 + ql;
    const int64_t o = (int64_t)Q * g0 + (int64_t)q * G + gl;
    if (!valid[g0 + gl]) { dot[o] = 0.0f; cosv[o] = 0.0f; continue; }
    const float* const kr = key + ((int64_t)b * Qk + key_row(key_index, g0 + gl, g0 + G, Qk)) * C;
    const float* const rr_ = s_ref + ql * (C + 1);
    float d = 0.0f, rr = 0.0f, kk = 0.0f;
    for (int c = 0; c < C; ++c) {                 // ascending channel order, one rounding per term
      const float r = rr_[c], kv = kr[c];
      d = fmaf(r, kv, d);
      rr = fmaf(r, r, rr);
      kk = fmaf(kv, kv, kk);
    }
    const float nr = sqrtf(rr), nk = sqrtf(kk);
    dot[o] = d;
    cosv[o] = d / (fmaxf(nr, kNormEps) * fmaxf(nk, kNormEps));
    if (gl == first_valid) ref_norm[(int64_t)b * Q + q] = nr;
    if (q == 0) key_norm[g0 + gl] = nk;
  }
}

// ---- loss ---------------------------------------------------------------------------------------------------------------------
constexpr int kLT = 256, kLW = kLT / 64;
constexpr int kStats = 6;                         // item_stats: term, aux term, max neg, max -pos, sigma / S_neg, sigma / S_pos

// sum over the workgroup in a fixed tree; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* s_red) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_red[tid] = v;
  __syncthreads();
  for (int s = kLT / 2; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] = s_red[tid] + s_red[tid + s];
    __syncthreads();
  }
  return s_red[0];
}
__device__ __forceinline__ float block_max(float v, double* s_red) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_red[tid] = (double)v;
  __syncthreads();
  for (int s = kLT / 2; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] = fmax(s_red[tid], s_red[tid + s]);
    __syncthreads();
  }
  return (float)s_red[0];
}

__global__ void __launch_bounds__(kLT)
reid_loss_kernel(const float* __restrict__ dot, const float* __restrict__ cosv, const uint8_t* __restrict__ mpos,
                 const uint8_t* __restrict__ mneg, const int32_t* __restrict__ meta, const int32_t* __restrict__ ranks, BatchOffsets go,
                 int batch, int Q, uint8_t* __restrict__ roles, double* __restrict__ stats) {
  __shared__ uint8_t s_flag[REID_HIP_MAX_QUERIES];           // per rank among the negatives: sampled
  __shared__ double s_red[kLT];
  __shared__ int s_wave[kLW];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t* const m = meta + (int64_t)i * REID_HIP_META;
  const int b = min(max(m[0], 0), batch - 1);
  const int g0 = go.off[b], G = go.off[b + 1] - g0;
  const int gl = m[1] - g0, roff = m[2], rcnt = m[3], n_aux = m[4];
  if (G <= 0 || gl < 0 || gl >= G) {              // (a malformed item: nothing is read through it)
    for (int q = tid; q < Q; q += kLT) roles[(int64_t)i * Q + q] = 0;
    if (tid < kStats) stats[(int64_t)i * kStats + tid] = 0.0;
    return;
  }
  const int64_t base = (int64_t)Q * g0 + gl;
  for (int q = tid; q < Q; q += kLT) s_flag[q] = 0;
  __syncthreads();
  for (int j = tid; j < rcnt; j += kLT) {
    const int r = ranks[roff + j];
    if (r >= 0 && r < Q) s_flag[r] = 1;
  }
  __syncthreads();

  float mn = -INFINITY, mp = -INFINITY;
  for (int q = tid; q < Q; q += kLT) {
    const int64_t o = base + (int64_t)q * G;
    const float d = dot[o];
    if (mneg[o] == 0) mn = fmaxf(mn, d);
    if (mpos[o] & 1) mp = fmaxf(mp, -d);
  }
  mn = block_max(mn, s_red);
  mp = block_max(mp, s_red);

  double sn = 0.0, sp = 0.0, aux = 0.0;
  int rank_base = 0;
  for (int q0 = 0; q0 < Q; q0 += kLT) {
    const int q = q0 + tid;
    const int64_t o = base + (int64_t)q * G;
    const bool in = q < Q;
    const bool isneg = in && mneg[o] == 0, ispos = in && (mpos[o] & 1);
    const unsigned long long bal = __ballot(isneg);
    __syncthreads();
    if (lane == 0) s_wave[wv] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kLW; ++w) {
      const int c = s_wave[w];
      if (w < wv) before += c;
      total += c;
    }
    // the rank of a negative in ascending query order: the order of ref_embeds[~mask]
    const int rank = rank_base + before + __popcll(bal & ((1ull << lane) - 1ull));
    const bool sampled = isneg && s_flag[rank] != 0;
    if (in) {
      roles[(int64_t)i * Q + q] = (uint8_t)((ispos ? 1 : 0) | (isneg ? 2 : 0) | (sampled ? 4 : 0));
      const float d = dot[o], c = cosv[o];
      if (isneg) sn += (double)expf(d - mn);
      if (ispos) {
        sp += (double)expf(-d - mp);
        aux += (double)((c - 1.0f) * (c - 1.0f));
      }
      if (sampled) aux += (double)(c * c);
    }
    rank_base += total;
  }
  sn = block_sum(sn, s_red);
  sp = block_sum(sp, s_red);
  aux = block_sum(aux, s_red);
  if (tid == 0) {
    double term = 0.0, sig = 0.0;
    if (sn > 0.0 && sp > 0.0) {                   // log(1 + S_neg * S_pos), the maxima taken out
      const double t = (double)mn + (double)mp + log(sn) + log(sp);
      term = fmax(t, 0.0) + log1p(exp(-fabs(t)));
      sig = 1.0 / (1.0 + exp(-t));
    }
    double* const s = stats + (int64_t)i * kStats;
    s[0] = term;
    s[1] = aux / (double)n_aux;                   // (the mean of nothing is NaN, as in the reference)
    s[2] = (double)mn;
    s[3] = (double)mp;
    s[4] = sn > 0.0 ? sig / sn : 0.0;
    s[5] = sp > 0.0 ? sig / sp : 0.0;
  }
}

__global__ void reid_loss_sum_kernel(const double* __restrict__ stats, int n, float* __restrict__ losses) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.0, x = 0.0;
  for (int i = 0; i < n; ++i) {                   // item order
    a = a + stats[(int64_t)i * kStats];
    x = x + stats[(int64_t)i * kStats + 1];
  }
  losses[0] = (float)(a / (double)n);
  losses[1] = (float)(x / (double)n);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// coef[0][i, q] = d L / d dot + (d L / d cos) / (max(|r|, eps) max(|k|, eps)): what multiplies the OTHER vector;
// coef[1][i, q] = (d L / d cos) * cos: what, over the squared own norm, multiplies the own vector (the normalisation's derivative)
__global__ void __launch_bounds__(256)
reid_coef_kernel(const float* __restrict__ dot, const float* __restrict__ cosv, const float* __restrict__ ref_norm,
                 const float* __restrict__ key_norm, const uint8_t* __restrict__ roles, const double* __restrict__ stats,
                 const int32_t* __restrict__ meta, const float* __restrict__ grad, BatchOffsets go, int batch, int Q, int n_items,
                 float* __restrict__ coef) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)n_items * Q) return;
  const int i = (int)(e / Q), q = (int)(e - (int64_t)i * Q);
  const int32_t* const m = meta + (int64_t)i * REID_HIP_META;
  const int b = min(max(m[0], 0), batch - 1);
  const int g0 = go.off[b], G = go.off[b + 1] - g0, gl = m[1] - g0;
  const uint8_t role = roles[e];
  float a = 0.0f, own = 0.0f;
  if (role != 0 && G > 0 && gl >= 0 && gl < G) {
    const int64_t o = (int64_t)Q * g0 + (int64_t)q * G + gl;
    const double* const s = stats + (int64_t)i * kStats;
    const float d = dot[o], c = cosv[o];
    const float inv_n = 1.0f / (float)n_items;
    float gd = 0.0f;
    if (role & 2) gd = gd + (float)s[4] * expf(d - (float)s[2]);
    if (role & 1) gd = gd - (float)s[5] * expf(-d - (float)s[3]);
    gd = gd * (grad[0] * inv_n);
    float ec = 0.0f;
    if (role & 1) ec = ec + (c - 1.0f);
    if (role & 4) ec = ec + c;
    const float gc = ec * (2.0f / (float)m[4]) * (grad[1] * inv_n);
    const float nr = fmaxf(ref_norm[(int64_t)b * Q + q], kNormEps), nk = fmaxf(key_norm[m[1]], kNormEps);
    a = gd + gc / (nr * nk);
    own = gc * c;
  }
  coef[e] = a;
  coef[(int64_t)n_items * Q + e] = own;
}

// grad_ref[b, q, :] = sum over the image's items (ascending) of coef0 * key row  -  [|r| > eps] (sum coef1) / |r|^2 * r: one wave a row
__global__ void __launch_bounds__(256)
reid_grad_ref_kernel(const float* __restrict__ ref, const float* __restrict__ key, const long long* __restrict__ key_index,
                     const float* __restrict__ ref_norm, const int32_t* __restrict__ meta, const float* __restrict__ coef,
                     BatchOffsets io, int n_targets, int Q, int Qk, int C, int n_items, float* __restrict__ grad_ref) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= Q) return;
  const int i0 = io.off[b], i1 = io.off[b + 1];
  float acc[REID_HIP_MAX_DIM / 64];
#pragma unroll
  for (int j = 0; j < REID_HIP_MAX_DIM / 64; ++j) acc[j] = 0.0f;
  float own = 0.0f;
  for (int i = i0; i < i1; ++i) {
    const float a = coef[(int64_t)i * Q + q];
    own = own + coef[((int64_t)n_items + i) * Q + q];
    const float* const kr = key + ((int64_t)b * Qk + key_row(key_index, meta[(int64_t)i * REID_HIP_META + 1], n_targets, Qk)) * C;
#pragma unroll
    for (int j = 0; j < REID_HIP_MAX_DIM / 64; ++j)
      if (j * 64 < C) acc[j] = fmaf(a, kr[j * 64 + lane], acc[j]);
  }
  float f = 0.0f;
  if (i1 > i0) {
    const float nr = ref_norm[(int64_t)b * Q + q];
    f = nr > kNormEps ? -own / (nr * nr) : 0.0f;
  }
  const int64_t row = ((int64_t)b * Q + q) * C;
#pragma unroll
  for (int j = 0; j < REID_HIP_MAX_DIM / 64; ++j)
    if (j * 64 < C) grad_ref[row + j * 64 + lane] = fmaf(f, ref[row + j * 64 + lane], acc[j]);
}

// key_item_grad[i, :] = sum over q of coef0 * reference row  -  [|k| > eps] (sum coef1) / |k|^2 * k: one workgroup an item, the queries
// dealt to 512 / C groups of C threads (ascending within a group), the groups added in ascending order
constexpr int kKT = 512;
__global__ void __launch_bounds__(kKT)
reid_grad_key_item_kernel(const float* __restrict__ ref, const float* __restrict__ key, const long long* __restrict__ key_index,
                          const float* __restrict__ key_norm, const int32_t* __restrict__ meta, const float* __restrict__ coef,
                          int batch, int n_targets, int Q, int Qk, int C, int n_items, float* __restrict__ key_item_grad) {
  __shared__ float s_part[kKT];
  __shared__ float s_own[kKT / 64];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int32_t* const m = meta + (int64_t)i * REID_HIP_META;
  const int b = min(max(m[0], 0), batch - 1);
  const int groups = kKT / C, grp = tid / C, c = tid - grp * C;
  float acc = 0.0f, own = 0.0f;
  if (grp < groups) {
    for (int q = grp; q < Q; q += groups) {
      acc = fmaf(coef[(int64_t)i * Q + q], ref[((int64_t)b * Q + q) * C + c], acc);
      own = own + coef[((int64_t)n_items + i) * Q + q];
    }
  }
  s_part[tid] = acc;
  if (grp < groups && c == 0) s_own[grp] = own;
  __syncthreads();
  if (tid < C) {
    float total = 0.0f, o = 0.0f;
    for (int g = 0; g < groups; ++g) {
      total = total + s_part[g * C + tid];
      o = o + s_own[g];
    }
    const float nk = key_norm[min(max(m[1], 0), n_targets - 1)];
    const float f = nk > kNormEps ? -o / (nk * nk) : 0.0f;
    const float kv = key[((int64_t)b * Qk + key_row(key_index, m[1], n_targets, Qk)) * C + tid];
    key_item_grad[(int64_t)i * C + tid] = fmaf(f, kv, total);
  }
}

// grad_key[b, k, :] = the item gradients of the image's items on key row k, added in ascending item order (0 elsewhere)
__global__ void __launch_bounds__(256)
reid_grad_key_kernel(const float* __restrict__ key_item_grad, const long long* __restrict__ key_index, const int32_t* __restrict__ meta,
                     BatchOffsets io, int batch, int n_targets, int Qk, int C, float* __restrict__ grad_key) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)batch * Qk * C) return;
  const int c = (int)(e % C);
  const int64_t row = e / C;
  const int b = (int)(row / Qk), k = (int)(row - (int64_t)b * Qk);
  float sum = 0.0f;
  for (int i = io.off[b]; i < io.off[b + 1]; ++i)
    if (key_row(key_index, meta[(int64_t)i * REID_HIP_META + 1], n_targets, Qk) == k) sum = sum + key_item_grad[(int64_t)i * C + c];
  grad_key[e] = sum;
}

bool bad_dim(int dim) { return dim <= 0 || dim > REID_HIP_MAX_DIM || dim % 64 != 0; }

}  // namespace
}  // namespace reid

extern "C" int ota_reid_select_hip(float* cost, const float* iou, const uint8_t* flags, const uint8_t* valid, const long long* key_index,
                               const int32_t* gt_off, int batch, int num_queries, int num_key_queries, int max_rounds,
                               uint8_t* matching_pos, uint8_t* matching_neg, int32_t* counts, int32_t* status, void* stream) {
  msda::BatchOffsets go;
  int max_g = 0;
  if (num_queries < reid::kNegCandidates || num_queries > REID_HIP_MAX_QUERIES || num_key_queries <= 0)
    return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_select_hip: num_queries has to be in [100, REID_HIP_MAX_QUERIES], num_key_queries positive");
  if (int rc = msda::fill_offsets(gt_off, batch, 1, &go, &max_g)) return rc;
  if (max_g > msda::kMaxGt) return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_select_hip: more than 4096 targets in one image");
  if ((int64_t)num_queries * go.off[batch] > 0x7fffffffLL) return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_select_hip: num_queries * targets too large");
  if (!status) return msda::set_error(OTA_ERR_NULL_POINTER, "ota_reid_select_hip: null pointer");
  if (max_g > 0 && (!cost || !iou || !flags || !valid || !key_index || !matching_pos || !matching_neg || !counts))
    return msda::set_error(OTA_ERR_NULL_POINTER, "ota_reid_select_hip: null pointer");
  hipLaunchKernelGGL(reid::reid_select_kernel, dim3((unsigned)batch), dim3(reid::kST), 0, static_cast<hipStream_t>(stream), cost, iou,
                     flags, valid, key_index, go, num_queries, num_key_queries, max_rounds, matching_pos, matching_neg, counts, status);
  return msda::launch_status();
}

extern "C" int ota_reid_scores_hip_f32(const float* ref_embeds, const float* key_embeds, const long long* key_index, const uint8_t* valid,
                                   const int32_t* gt_off, int batch, int num_queries, int num_key_queries, int dim, float* dot,
                                   float* cos, float* ref_norm, float* key_norm, void* stream) {
  msda::BatchOffsets go;
  int max_g = 0;
  if (num_queries <= 0 || num_key_queries <= 0 || reid::bad_dim(dim))
    return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_scores_hip_f32: dimensions (dim: a multiple of 64 up to REID_HIP_MAX_DIM)");
  if (int rc = msda::fill_offsets(gt_off, batch, 1, &go, &max_g)) return rc;
  if ((int64_t)num_queries * go.off[batch] > 0x7fffffffLL) return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_scores_hip_f32: num_queries * targets too large");
  if (max_g == 0) return 0;
  if (!ref_embeds || !key_embeds || !key_index || !valid || !dot || !cos || !ref_norm || !key_norm)
    return msda::set_error(OTA_ERR_NULL_POINTER, "ota_reid_scores_hip_f32: null pointer");
  hipLaunchKernelGGL(reid::reid_scores_kernel, dim3((unsigned)msda::ceil_div(num_queries, reid::kTQ), (unsigned)batch), dim3(reid::kScT), 0,
                     static_cast<hipStream_t>(stream), ref_embeds, key_embeds, key_index, valid, go, num_queries, num_key_queries, dim,
                     dot, cos, ref_norm, key_norm);
  return msda::launch_status();
}

extern "C" int ota_reid_loss_hip_f32(const float* dot, const float* cos, const uint8_t* matching_pos, const uint8_t* matching_neg,
                                 const int32_t* item_meta, const int32_t* ranks, const int32_t* gt_off, int batch, int num_queries,
                                 int num_items, uint8_t* roles, double* item_stats, float* losses, void* stream) {
  msda::BatchOffsets go;
  int max_g = 0;
  if (num_queries <= 0 || num_queries > REID_HIP_MAX_QUERIES || num_items <= 0)
    return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_loss_hip_f32: num_queries in [1, REID_HIP_MAX_QUERIES], at least one item");
  if (int rc = msda::fill_offsets(gt_off, batch, 1, &go, &max_g)) return rc;
  if (num_items > go.off[batch]) return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_loss_hip_f32: more items than targets");
  if (!dot || !cos || !matching_pos || !matching_neg || !item_meta || !ranks || !roles || !item_stats || !losses)
    return msda::set_error(OTA_ERR_NULL_POINTER, "ota_reid_loss_hip_f32: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(reid::reid_loss_kernel, dim3((unsigned)num_items), dim3(reid::kLT), 0, s, dot, cos, matching_pos, matching_neg,
                     item_meta, ranks, go, batch, num_queries, roles, item_stats);
  hipLaunchKernelGGL(reid::reid_loss_sum_kernel, dim3(1), dim3(64), 0, s, item_stats, num_items, losses);
  return msda::launch_status();
}

extern "C" int ota_reid_loss_bwd_hip_f32(const float* ref_embeds, const float* key_embeds, const long long* key_index, const float* dot,
                                     const float* cos, const float* ref_norm, const float* key_norm, const uint8_t* roles,
                                     const double* item_stats, const int32_t* item_meta, const int32_t* item_off,
                                     const float* grad_losses, const int32_t* gt_off, int batch, int num_queries, int num_key_queries,
                                     int dim, int num_items, float* coef, float* key_item_grad, float* grad_ref, float* grad_key,
                                     void* stream) {
  msda::BatchOffsets go, io;
  int max_g = 0, max_i = 0;
  if (num_queries <= 0 || num_key_queries <= 0 || num_items <= 0 || reid::bad_dim(dim))
    return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_loss_bwd_hip_f32: dimensions (dim: a multiple of 64 up to REID_HIP_MAX_DIM)");
  if (int rc = msda::fill_offsets(gt_off, batch, 1, &go, &max_g)) return rc;
  if (int rc = msda::fill_offsets(item_off, batch, 1, &io, &max_i)) return rc;
  if (io.off[batch] != num_items) return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_loss_bwd_hip_f32: item_off does not end at num_items");
  for (int b = 0; b < batch; ++b)
    if (io.off[b + 1] - io.off[b] > go.off[b + 1] - go.off[b])
      return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_loss_bwd_hip_f32: an image has more items than targets");
  if (!ref_embeds || !key_embeds || !key_index || !dot || !cos || !ref_norm || !key_norm || !roles || !item_stats || !item_meta ||
      !grad_losses || !coef || !key_item_grad || !grad_ref || !grad_key)
    return msda::set_error(OTA_ERR_NULL_POINTER, "ota_reid_loss_bwd_hip_f32: null pointer");
  const int64_t nq = (int64_t)num_items * num_queries, nk = (int64_t)batch * num_key_queries * dim;
  if (msda::ceil_div(nq, (int64_t)256) > 0x7fffffffLL || msda::ceil_div(nk, (int64_t)256) > 0x7fffffffLL)
    return msda::set_error(OTA_ERR_BAD_DIMS, "ota_reid_loss_bwd_hip_f32: too large");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(reid::reid_coef_kernel, dim3((unsigned)msda::ceil_div(nq, (int64_t)256)), dim3(256), 0, s, dot, cos, ref_norm, key_norm,
                     roles, item_stats, item_meta, grad_losses, go, batch, num_queries, num_items, coef);
  hipLaunchKernelGGL(reid::reid_grad_ref_kernel, dim3((unsigned)msda::ceil_div(num_queries, 4), (unsigned)batch), dim3(256), 0, s, ref_embeds,
                     key_embeds, key_index, ref_norm, item_meta, coef, io, go.off[batch], num_queries, num_key_queries, dim, num_items, grad_ref);
  hipLaunchKernelGGL(reid::reid_grad_key_item_kernel, dim3((unsigned)num_items), dim3(reid::kKT), 0, s, ref_embeds, key_embeds, key_index,
                     key_norm, item_meta, coef, batch, go.off[batch], num_queries, num_key_queries, dim, num_items, key_item_grad);
  hipLaunchKernelGGL(reid::reid_grad_key_kernel, dim3((unsigned)msda::ceil_div(nk, (int64_t)256)), dim3(256), 0, s, key_item_grad, key_index,
                     item_meta, io, batch, go.off[batch], num_key_queries, dim, grad_key);
  return msda::launch_status();
}
