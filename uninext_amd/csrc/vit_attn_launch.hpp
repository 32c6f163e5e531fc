// What vit_attn.hip lends to the training route (vit_attn_bwd.hip): the geometry check, the size of the relative-position terms,
// the divide-by-q_w constant and the launch of the rel_terms kernel.  Internal: host only, not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace vit_attn {

// 0, or a negative PATCH_EMBED_ERR_* (message set)
int geometry(int batch, int num_heads, int q_h, int q_w, int head_dim);
// bytes of rel[batch * num_heads, q_h + q_w, roundup(S, 32)]: the forward's whole workspace (at least 256)
size_t rel_bytes(int batch, int num_heads, int q_h, int q_w);
// x / q_w == __umulhi(x, div_magic(q_w)) inside the geometry limits (q_w == 1: unused)
unsigned div_magic(int q_w);
// enqueues rel_terms<head_dim> (head_dim 64 or 80, geometry checked by the caller); 0 or the launch's status
int launch_rel_terms(int head_dim, hipStream_t stream, const float* qkv, const float* rel_h_table, const float* rel_w_table, int batch,
                     int num_heads, int q_h, int q_w, float* rel);

}  // namespace vit_attn
