/* dfdclip_explain.h — explanation entry points of libdfdclip_hip.so: what the decoder looked at.  Added beside the C ABI of
 * dfdclip.h WITHOUT a new DFD_ABI_VERSION (still 17): nothing in dfdclip.h or dfdclip_ext.h changed.  A library built before
 * them lacks the symbols, which the loader reports by name.  Conventions (device pointers, `stream`, return codes,
 * dfd_last_error, dfd_kv_layout_t) are dfdclip.h's.
 *
 * They live in a header of their own because the function lists of dfdclip.h and dfdclip_ext.h are pinned, each to the
 * guard-band module that covers it (tests/test_guarded_cpu.py, tests/test_fp8_policy_cpu.py); the functions here are covered
 * by tests/test_hip_guarded_attnmap.py under the same rule (tests/test_attnmap_cpu.py checks it).  The Python binding lists
 * them in capi.EXPLAIN_SIGNATURES. */
#ifndef DFDCLIP_EXPLAIN_H
#define DFDCLIP_EXPLAIN_H

#include <stdint.h>

#include "dfdclip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The per-key weight that dfd_decoder_attn_fwd applies to v, for one decoder layer:
 *   aff[b, h, s] = ½·(w_softmax + w_coda),   mix[b, h, :] = Σ_s aff[b, h, s] · v[b, s, h, :]
 *   w_softmax = exp(q_s·k/√d − max) / sumexp with (max, sumexp) = stats[b, h, :] as dfd_decoder_attn_fwd wrote them, or
 *               ext_weights[b, h, s] when ext_weights is given (attn_mode; stats is then not read and may be NULL)
 *   w_coda    = tanh(q_c·k/√d) · 2σ(−‖q_c − k‖₁/√d)      (can be negative)
 * Keys of padded frames (frame_mask[b, t] == 0) get exactly 0.0f in both branches.  The three sums of a key row are formed
 * by the forward's own code, so they carry the forward's bits.
 *   q           f32 [B, heads, 2*d]; k kv_dtype through `layout` as for dfd_decoder_attn_fwd (NULL = dense); d == 64
 *   frame_mask  u8 [B, T], S == T * patches
 *   aff         f32 [B, heads, S]
 *   branches    f32 [2, B, heads, S] or NULL: w_softmax, then w_coda, without the ½
 * One pass over K: V is not read, there is no workspace, and every element of aff (and branches) is written exactly
 * once, padded keys included. */
int dfd_decoder_attn_map(const float* q, const void* k, int kv_dtype, const dfd_kv_layout_t* layout, const uint8_t* frame_mask,
                         const float* stats, const float* ext_weights, float* aff, float* branches, int B, int T, int patches,
                         int heads, int d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_EXPLAIN_H */
