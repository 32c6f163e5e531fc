// Decoder prediction heads: class logits, boxes, IoU logit and the mask head's parameters of every query from one level's hidden
// states -- see include/dynmask_hip.h (pred_heads_hip_f32).
//
// All heads read the same [B, Q, 256] rows.  A workgroup (4 waves) owns a tile of 32 rows of ONE image (the class weight is the
// image's text) in LDS and runs the row-tile routine of row_tile.hpp on it:
//
//   class       acc = X tokens[b]^T, the bounded routine (T <= 256 weight rows); / scale, + token_bias, clamp; stored [B, Q, T];
//   IoU         one butterfly sum per row, from the tile as loaded;
//   box         two `linear` steps with ReLU (they overwrite the tile), the 256 -> 4 layer as four butterfly sums per row,
//               + inverse_sigmoid(reference) on the first ref_dim columns, the precise sigmoid;
//   controller  two `linear` steps with ReLU, then the bounded routine with P <= 256 weight rows, + bias; stored [B, Q, P].
//
// Two grids.  "split": the branch (class / IoU + box / controller) is the grid's z, so a workgroup streams at most three weights
// and no step needs the tile after another branch overwrote it.  "tile": one workgroup per tile runs the branches in that order and
// fetches the tile a second time before the controller.  Both compute every number in the same order: their results are bitwise
// equal.  Exact fp32, fixed summation orders, no atomics: bitwise repeatable, and a row's result does not depend on its place.
#include "../../include/dynmask_hip.h"

#include <math.h>

#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "row_tile.hpp"

namespace phead {

using namespace row_tile;
using msda::wave_sum;

constexpr int kClass = 0, kBox = 1, kCtrl = 2;
constexpr float kEps = 1e-5f;           // inverse_sigmoid's

struct Mlp {
  const float* __restrict__ w1;
  const float* __restrict__ b1;
  const float* __restrict__ w2;
  const float* __restrict__ b2;
  const float* __restrict__ w3;
  const float* __restrict__ b3;
};

struct Args {
  const float* __restrict__ hs;              // [B, Q, 256]
  const float* __restrict__ tokens;          // [B | 1, T, 256]
  const float* __restrict__ token_bias;      // [B | 1, T]
  long long tokens_stride, token_bias_stride;
  const float* __restrict__ scale;           // one float, or NULL
  float clamp;
  const float* __restrict__ reference;       // [B, Q, ref_dim]
  int ref_dim;
  Mlp box;
  const float* __restrict__ iou_w;           // [256], or NULL
  const float* __restrict__ iou_b;
  Mlp ctrl;                                  // w3 [P, 256]; used when params is not NULL
  int P, T;
  long long Q;
  float* __restrict__ logits;                // [B, Q, T]
  float* __restrict__ boxes;                 // [B, Q, 4]
  float* __restrict__ iou;                   // [B, Q], or NULL
  float* __restrict__ params;                // [B, Q, P], or NULL
};

// rows [0, live) of `rows` into the tile, zeros behind them; wave w fetches rows w, w + 4, ...
__device__ __forceinline__ void load_tile(float (*Xs)[kPitch], const float* __restrict__ rows, int live, int tid) {
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int row = wv + r * (kThreads / 64);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < live) v = *reinterpret_cast<const f32x4*>(rows + (long long)row * kD + lane * 4);
    *reinterpret_cast<f32x4*>(&Xs[row][lane * 4]) = v;
  }
}

// out[row, col] = f(acc, col) for the live rows and the columns below n_out; out is the tile's first row, n_out floats a row
template <typename F>
__device__ __forceinline__ void store_acc(const f32x16 (&acc)[2], float* __restrict__ out, int n_out, int live, int tid, F f) {
  const int lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int col = wv * 64 + nt * 32 + r32;
    if (col >= n_out) continue;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int row = acc_row(v) + 4 * half;
      if (row < live) out[(long long)row * n_out + col] = f(acc[nt][v], col);
    }
  }
}

__device__ __forceinline__ float inverse_sigmoid(float x) {
  x = fminf(fmaxf(x, 0.f), 1.f);
  return logf(__fdiv_rn(fmaxf(x, kEps), fmaxf(1.f - x, kEps)));
}

// Rows [first, first + 32) of image blockIdx.y; SPLIT: the branch blockIdx.z of them.
template <bool SPLIT>
__global__ void __launch_bounds__(kThreads) heads(Args a) {
  __shared__ __attribute__((aligned(16))) float Xs[kRows][kPitch];
  __shared__ __attribute__((aligned(16))) float Ws[kD][kWPitch];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.y, branch = SPLIT ? (int)blockIdx.z : -1;
  const long long first = (long long)blockIdx.x * kRows, n0 = (long long)b * a.Q + first;
  const int live = (int)(a.Q - first < kRows ? a.Q - first : kRows);
  const float* __restrict__ rows = a.hs + n0 * kD;
  load_tile(Xs, rows, live, tid);

  if (!SPLIT || branch == kClass) {
    f32x16 acc[2];
    matmul_tile<true>(acc, Xs, Ws, a.tokens + b * a.tokens_stride, a.T, tid);
    const float sc = a.scale ? a.scale[0] : 1.f, clamp = a.clamp;
    const float* __restrict__ tb = a.token_bias + b * a.token_bias_stride;
    store_acc(acc, a.logits + n0 * a.T, a.T, live, tid, [=](float y, int col) {
      const float s = __fdiv_rn(y, sc) + tb[col];
      return clamp > 0.f ? fminf(fmaxf(s, -clamp), clamp) : s;
    });
  }

  if (!SPLIT || branch == kBox) {
    if (a.iou) {                           // rows this wave loaded itself
      const f32x4 wi = *reinterpret_cast<const f32x4*>(a.iou_w + lane * 4);
#pragma unroll
      for (int r = 0; r < kRowsPerWave; ++r) {
        const int row = wv + r * (kThreads / 64);
        if (row >= live) continue;         // wave-uniform
        const float s = wave_sum(dot4(*reinterpret_cast<const f32x4*>(&Xs[row][lane * 4]), wi)) + a.iou_b[0];
        if (lane == 0) a.iou[n0 + row] = s;
      }
    }
    linear_tile<true>(Xs, Ws, a.box.w1, a.box.b1, tid);
    linear_tile<true>(Xs, Ws, a.box.w2, a.box.b2, tid);
    f32x4 w3r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) w3r[c] = *reinterpret_cast<const f32x4*>(a.box.w3 + c * kD + lane * 4);
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
      const int row = wv + r * (kThreads / 64);
      if (row >= live) continue;           // wave-uniform
      const f32x4 h = *reinterpret_cast<const f32x4*>(&Xs[row][lane * 4]);
      f32x4 out;
#pragma unroll
      for (int c = 0; c < 4; ++c) out[c] = wave_sum(dot4(h, w3r[c])) + a.box.b3[c];
      if (lane == 0) {
        const float* __restrict__ ref = a.reference + (n0 + row) * a.ref_dim;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (c < a.ref_dim) out[c] += inverse_sigmoid(ref[c]);
          out[c] = 1.f / (1.f + expf(-out[c]));
        }
        *reinterpret_cast<f32x4*>(a.boxes + (n0 + row) * 4) = out;
      }
    }
  }

  if ((!SPLIT || branch == kCtrl) && a.params) {
    if (!SPLIT) {                          // the box MLP overwrote the tile
      __syncthreads();
      load_tile(Xs, rows, live, tid);
    }
    linear_tile<true>(Xs, Ws, a.ctrl.w1, a.ctrl.b1, tid);
    linear_tile<true>(Xs, Ws, a.ctrl.w2, a.ctrl.b2, tid);
    f32x16 acc[2];
    matmul_tile<true>(acc, Xs, Ws, a.ctrl.w3, a.P, tid);
    const float* __restrict__ b3 = a.ctrl.b3;
    store_acc(acc, a.params + n0 * a.P, a.P, live, tid, [=](float y, int col) { return y + b3[col]; });
  }
}

}  // namespace phead

extern "C" {

static const char* g_pred_heads_last = "";
static int g_pred_heads_variant = 0;

const char* pred_heads_hip_last_kernel(void) { return g_pred_heads_last; }

int pred_heads_hip_set_variant(int variant) {
  if (variant < 0 || variant > 2) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "pred_heads: variant must be 0 (auto), 1 (split) or 2 (tile)");
  g_pred_heads_variant = variant;
  return 0;
}

int pred_heads_hip_f32(const float* hs, const float* tokens, long long tokens_stride, const float* token_bias,
                       long long token_bias_stride, const float* scale, float clamp, const float* reference, int ref_dim,
                       const float* box_w1, const float* box_b1, const float* box_w2, const float* box_b2, const float* box_w3,
                       const float* box_b3, const float* iou_weight, const float* iou_bias, const float* ctrl_w1,
                       const float* ctrl_b1, const float* ctrl_w2, const float* ctrl_b2, const float* ctrl_w3, const float* ctrl_b3,
                       int P, int batch, long long Q, int T, int d_model, float* logits, float* boxes, float* iou, float* params,
                       void* stream) {
  if (batch < 0 || Q < 0 || d_model <= 0) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "pred_heads: bad dimensions");
  if (d_model != phead::kD) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "pred_heads: d_model must be 256");
  if (batch > 65535 || Q >= (1ll << 31)) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "pred_heads: problem too large");
  if (T < 1) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "pred_heads: T must be at least 1");
  if (T > PRED_HEADS_HIP_MAX_TOKENS) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "pred_heads: T must be at most 256");
  if (ref_dim != 2 && ref_dim != 4) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "pred_heads: ref_dim must be 2 or 4");
  if (params && P < 1) return msda::set_error(DYNMASK_ERR_BAD_DIMS, "pred_heads: P must be at least 1");
  if (params && P > PRED_HEADS_HIP_MAX_PARAMS) return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "pred_heads: P must be at most 256");
  if (tokens_stride < 0 || token_bias_stride < 0 || tokens_stride % 4 != 0)
    return msda::set_error(DYNMASK_ERR_BAD_DIMS, "pred_heads: token strides must be >= 0, the tokens' a multiple of 4");
  if (batch == 0 || Q == 0) return 0;
  if (!hs || !tokens || !token_bias || !reference || !box_w1 || !box_b1 || !box_w2 || !box_b2 || !box_w3 || !box_b3 || !logits ||
      !boxes || (iou && (!iou_weight || !iou_bias)) ||
      (params && (!ctrl_w1 || !ctrl_b1 || !ctrl_w2 || !ctrl_b2 || !ctrl_w3 || !ctrl_b3)))
    return msda::set_error(DYNMASK_ERR_NULL_POINTER, "pred_heads: null pointer argument");
  if (!msda::aligned16({hs, tokens, box_w1, box_w2, box_w3, boxes, iou ? iou_weight : nullptr, params ? ctrl_w1 : nullptr,
                        params ? ctrl_w2 : nullptr, params ? ctrl_w3 : nullptr}))
    return msda::set_error(DYNMASK_ERR_UNSUPPORTED, "pred_heads: hs, tokens, weights and boxes must be 16-byte aligned");
  phead::Args a;
  a.hs = hs, a.tokens = tokens, a.token_bias = token_bias, a.tokens_stride = tokens_stride, a.token_bias_stride = token_bias_stride;
  a.scale = scale, a.clamp = clamp, a.reference = reference, a.ref_dim = ref_dim;
  a.box = phead::Mlp{box_w1, box_b1, box_w2, box_b2, box_w3, box_b3};
  a.iou_w = iou_weight, a.iou_b = iou_bias;
  a.ctrl = phead::Mlp{ctrl_w1, ctrl_b1, ctrl_w2, ctrl_b2, ctrl_w3, ctrl_b3};
  a.P = P, a.T = T, a.Q = Q, a.logits = logits, a.boxes = boxes, a.iou = iou, a.params = params;
  const bool split = g_pred_heads_variant != 2;      // auto: the split grid (profiles/r41_pred_heads.txt)
  const unsigned tiles = (unsigned)((Q + phead::kRows - 1) / phead::kRows);
  const dim3 block(phead::kThreads);
  if (split)
    hipLaunchKernelGGL(phead::heads<true>, dim3(tiles, (unsigned)batch, params ? 3u : 2u), block, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(phead::heads<false>, dim3(tiles, (unsigned)batch, 1u), block, 0, (hipStream_t)stream, a);
  if (const int e = msda::launch_status()) return e;
  g_pred_heads_last = split ? "pred_heads<split>" : "pred_heads<tile>";
  return 0;
}

}  // extern "C"
