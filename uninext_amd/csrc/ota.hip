// ota_cost_hip_f32 / ota_dynamic_k_hip (include/ota_hip.h): the simOTA assignment of HungarianMatcherVL.forward_ota on the
// device -- projects/UNINEXT/uninext/models/deformable_detr/matcher.py:313-447, util/box_ops.py:17-85.  gfx950.
//
// The outputs are integer index lists; every float that decides one is the float the reference's PyTorch composition
// forms: contraction is OFF for the whole file (an FMA rounds once where two kernels round twice), divisions are IEEE, and
// selections break ties towards the lowest index.  The assignment proper -- top-k, multiple claims, repair loop, with its
// in-place penalties and NaN conventions -- is dynamic_k.hpp's, shared with reid.hip.
//
// Mapping: the cost kernel is one thread per (query, target) pair, target fastest (coalesced stores; the threads of a wave
// share a few query rows and the target rows are a few hundred bytes).  The assignment is ONE 1024-thread workgroup per
// image: row operations (a query's claims, its cheapest target, penalties) are a thread per query, column operations (a
// target's top-k, its cheapest query) a wave per target with the lanes striding over the queries; phases are separated by
// workgroup barriers, nothing leaves the CU but the matrices themselves (L2-resident: 900 x G floats).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ota_hip.h"
#include "launch_glue.hpp"

#pragma clang fp contract(off)

#include "dynamic_k.hpp"

namespace msda {
namespace {

constexpr float kGiouWeight = 3.0f, kPriorPenalty = 100.0f, kBgPenalty = 10000.0f;   // matcher.py:338,340
constexpr float kCentreHalf = 2.5f / 32.0f;     // 1 * center_radius / expanded_strides (matcher.py:323,367): 0.078125, exact
constexpr int kTopIou = 10;                     // matcher.py:391

__global__ void __launch_bounds__(256)
ota_cost_kernel(const float* __restrict__ table, const float* __restrict__ boxes, const float* __restrict__ tgt_boxes,
                const uint8_t* __restrict__ posmap, BatchOffsets go, int Q, int T, float* __restrict__ cost,
                float* __restrict__ iou_out, uint8_t* __restrict__ flags) {
  const int b = blockIdx.y;
  const int g0 = go.off[b], G = go.off[b + 1] - g0;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)Q * G) return;
  const int q = (int)(i / G), k = (int)(i - (int64_t)q * G);
  // ---- classification: mean of the focal table over the target's positive tokens (matcher.py:332-334).  PyTorch's mean
  // is the sum times fl(1 / count); an empty selection gives 0 * inf = NaN, as there
  const float* row = table + ((int64_t)b * Q + q) * T;
  const uint8_t* pm = posmap + (int64_t)(g0 + k) * T;
  float sum = 0.0f;
  int cnt = 0;
  int t = 0;
  if ((T & 3) == 0 && (((uintptr_t)pm) & 3) == 0) {             // four map bytes at a time: most words are zero
    for (; t < T; t += 4) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(pm + t);
      if (w == 0u) continue;
      if (w & 0x000000ffu) { sum = sum + row[t]; ++cnt; }
      if (w & 0x0000ff00u) { sum = sum + row[t + 1]; ++cnt; }
      if (w & 0x00ff0000u) { sum = sum + row[t + 2]; ++cnt; }
      if (w & 0xff000000u) { sum = sum + row[t + 3]; ++cnt; }
    }
  } else {
    for (; t < T; ++t)
      if (pm[t]) { sum = sum + row[t]; ++cnt; }
  }
  const float cls = sum * (1.0f / (float)cnt);
  // ---- IoU and generalised IoU of the xyxy boxes (box_ops.py:17-23, torchvision box_iou, box_ops.py:62-85) --------------
  const float4 bq = *reinterpret_cast<const float4*>(boxes + ((int64_t)b * Q + q) * 4);
  const float4 g = *reinterpret_cast<const float4*>(tgt_boxes + (int64_t)(g0 + k) * 4);
  const float bx0 = bq.x - 0.5f * bq.z, by0 = bq.y - 0.5f * bq.w, bx1 = bq.x + 0.5f * bq.z, by1 = bq.y + 0.5f * bq.w;
  const float gx0 = g.x - 0.5f * g.z, gy0 = g.y - 0.5f * g.w, gx1 = g.x + 0.5f * g.z, gy1 = g.y + 0.5f * g.w;
  const float area1 = (bx1 - bx0) * (by1 - by0), area2 = (gx1 - gx0) * (gy1 - gy0);
  const float iw = fmaxf(fminf(bx1, gx1) - fmaxf(bx0, gx0), 0.0f), ih = fmaxf(fminf(by1, gy1) - fmaxf(by0, gy0), 0.0f);
  const float inter = iw * ih;
  const float uni = (area1 + area2) - inter;
  const float iou = inter / uni;
  const float hw = fmaxf(fmaxf(bx1, gx1) - fminf(bx0, gx0), 0.0f), hh = fmaxf(fmaxf(by1, gy1) - fminf(by0, gy0), 0.0f);
  const float hull = hw * hh;
  const float giou = iou - (hull - uni) / (hull + 1e-7f);
  // ---- centre prior (matcher.py:344-385): the query's centre strictly inside the box / inside the centre square --------
  const float cx = bq.x, cy = bq.y;
  const bool in_box = cx > gx0 && cx < gx1 && cy > gy0 && cy < gy1;
  const bool in_ctr = cx > g.x - kCentreHalf && cx < g.x + kCentreHalf && cy > g.y - kCentreHalf && cy < g.y + kCentreHalf;
  const int64_t o = (int64_t)Q * g0 + i;
  cost[o] = (cls + kGiouWeight * (-giou)) + kPriorPenalty * ((in_box && in_ctr) ? 0.0f : 1.0f);
  iou_out[o] = iou;
  // bit 1: a box of the pair fails the reference's `(boxes[:, 2:] >= boxes[:, :2]).all()` (util/box_ops.py:76-77; NaN fails it too):
  // the reference aborts the step with an AssertionError; the assignment kernel turns the bit into status 4 of the image
  const bool degenerate = !(bx1 >= bx0) || !(by1 >= by0) || !(gx1 >= gx0) || !(gy1 >= gy0);
  flags[o] = (uint8_t)(((in_box || in_ctr) ? 1 : 0) | (degenerate ? 2 : 0));
}

constexpr int kOT = 1024, kOW = kOT / 64;

__global__ void __launch_bounds__(kOT)
ota_dynamic_k_kernel(float* __restrict__ cost, const float* __restrict__ iou, const uint8_t* __restrict__ flags,
                     uint8_t* __restrict__ matching, BatchOffsets go, int Q, int max_rounds, int64_t* __restrict__ sel_query,
                     int64_t* __restrict__ sel_gt, int64_t* __restrict__ matched_query, int32_t* __restrict__ num_selected,
                     int32_t* __restrict__ status) {
  __shared__ uint8_t s_unmatched[kMaxGt];
  __shared__ int s_count[2];
  __shared__ int s_wave[kOW];
  const int b = blockIdx.x;
  const int g0 = go.off[b], G = go.off[b + 1] - g0;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (G <= 0) {
    if (tid == 0) { num_selected[b] = 0; status[b] = 0; }
    return;
  }
  float* const C = cost + (int64_t)Q * g0;
  const float* const I = iou + (int64_t)Q * g0;
  const uint8_t* const F = flags + (int64_t)Q * g0;
  uint8_t* const M = matching + (int64_t)Q * g0;

  // ---- (1) background penalty (matcher.py:340; fg_mask of :374: inside ANY box or ANY centre square) ---------------------
  int bad = 0;
  for (int q = tid; q < Q; q += kOT) {
    bool fg = false;
    for (int g = 0; g < G; ++g) {
      const uint8_t f = F[(int64_t)q * G + g];
      fg = fg || (f & 1) != 0;
      bad |= f & 2;
    }
    if (!fg)
      for (int g = 0; g < G; ++g) C[(int64_t)q * G + g] = C[(int64_t)q * G + g] + kBgPenalty;
  }
  const int degenerate = __syncthreads_or(bad) ? 4 : 0;      // (also the barrier behind this phase)

  // ---- (2) - (4) top-k, multiple claims, repair loop; M ends as the 0 / 1 matrix ------------------------------------------------
  const int st = dynamic_k<false, kOT>(C, I, M, nullptr, Q, G, min(Q, kTopIou), max_rounds, s_unmatched, s_count);

  // ---- (5) results (matcher.py:437-447): selected queries ascending with the first target of their row ------------------
  int base = 0;
  for (int q0 = 0; q0 < Q; q0 += kOT) {
    const int q = q0 + tid;
    int first = -1;
    if (q < Q)
      for (int g = G - 1; g >= 0; --g)
        if (M[(int64_t)q * G + g] & kMatch) first = g;          // matching[selected].max(1)[1]: the first maximum
    const unsigned long long bal = __ballot(first >= 0);
    if (lane == 0) s_wave[wv] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kOW; ++w) {
      const int c = s_wave[w];
      if (w < wv) before += c;
      total += c;
    }
    if (first >= 0) {
      const int pos = base + before + __popcll(bal & ((1ull << lane) - 1ull));
      sel_query[(int64_t)b * Q + pos] = q;
      sel_gt[(int64_t)b * Q + pos] = first;
    }
    base += total;
    __syncthreads();
  }
  // per target the cheapest query among its own (cost[matching == 0] += inf; torch.min(cost, dim=0)[1])
  for (int g = wv; g < G; g += kOW) {
    float bv = INFINITY;
    int bi = 0x7fffffff;
    for (int q = lane; q < Q; q += 64) {
      // (an entry outside the matching is cost + inf: +inf -- or NaN, which torch.min then returns even though it is not matched)
      const float c = C[(int64_t)q * G + g];
      const float v = nan_first((M[(int64_t)q * G + g] & kMatch) ? c : c + INFINITY);
      if (v < bv || (v == bv && q < bi)) { bv = v; bi = q; }
    }
    wave_ops::wave_argmin(bv, bi);
    if (lane == 0) matched_query[g0 + g] = bi == 0x7fffffff ? 0 : bi;   // (a column of +inf only: torch's argmin of all-inf is 0)
  }
  if (tid == 0) { num_selected[b] = base; status[b] = st | degenerate; }
}

}  // namespace
}  // namespace msda

extern "C" int ota_cost_hip_f32(const float* class_table, const float* boxes, const float* tgt_boxes, const uint8_t* positive_map,
                                const int32_t* gt_off, int batch, int num_queries, int num_tokens, float* cost, float* iou,
                                uint8_t* flags, void* stream) {
  msda::BatchOffsets go;
  int max_g = 0;
  if (num_queries < 0 || num_tokens < 0) return msda::set_error(OTA_ERR_BAD_DIMS, "ota_cost_hip_f32: negative dimension");
  if (int rc = msda::fill_offsets(gt_off, batch, 0, &go, &max_g)) return rc;
  if (batch == 0 || num_queries == 0 || max_g == 0) return 0;
  if (!class_table || !boxes || !tgt_boxes || !positive_map || !cost || !iou || !flags)
    return msda::set_error(OTA_ERR_NULL_POINTER, "ota_cost_hip_f32: null pointer");
  const int64_t n = (int64_t)num_queries * max_g, blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL || (int64_t)num_queries * go.off[batch] > 0x7fffffffLL)
    return msda::set_error(OTA_ERR_BAD_DIMS, "ota_cost_hip_f32: num_queries * targets too large");
  hipLaunchKernelGGL(msda::ota_cost_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(256), 0, static_cast<hipStream_t>(stream),
                     class_table, boxes, tgt_boxes, positive_map, go, num_queries, num_tokens, cost, iou, flags);
  return msda::launch_status();
}

extern "C" int ota_dynamic_k_hip(float* cost, const float* iou, const uint8_t* flags, uint8_t* matching, const int32_t* gt_off,
                                 int batch, int num_queries, int max_rounds, int64_t* sel_query, int64_t* sel_gt,
                                 int64_t* matched_query, int32_t* num_selected, int32_t* status, void* stream) {
  msda::BatchOffsets go;
  int max_g = 0;
  if (num_queries < 0) return msda::set_error(OTA_ERR_BAD_DIMS, "ota_dynamic_k_hip: negative dimension");
  if (int rc = msda::fill_offsets(gt_off, batch, 0, &go, &max_g)) return rc;
  if (batch == 0) return 0;
  if (max_g > msda::kMaxGt) return msda::set_error(OTA_ERR_BAD_DIMS, "ota_dynamic_k_hip: more than 4096 targets in one image");
  if (!num_selected || !status) return msda::set_error(OTA_ERR_NULL_POINTER, "ota_dynamic_k_hip: null pointer");
  if (max_g > 0 && num_queries > 0 && (!cost || !iou || !flags || !matching || !sel_query || !sel_gt || !matched_query))
    return msda::set_error(OTA_ERR_NULL_POINTER, "ota_dynamic_k_hip: null pointer");
  if (num_queries == 0) max_g = 0;
  msda::BatchOffsets run = go;
  if (max_g == 0)                      // nothing to assign anywhere: the kernel only writes the zero counts
    for (int b = 0; b <= batch; ++b) run.off[b] = 0;
  hipLaunchKernelGGL(msda::ota_dynamic_k_kernel, dim3((unsigned)batch), dim3(msda::kOT), 0, static_cast<hipStream_t>(stream), cost,
                     iou, flags, matching, run, num_queries, max_rounds, sel_query, sel_gt, matched_query, num_selected, status);
  return msda::launch_status();
}
