/* dfdclip_kvgather.h — the row gather of patch-masked training for libdfdclip_hip.so: `train_mode.patch_mask` keeps a subset
 * of patch positions of every tapped layer's K and V (the reference's src/models.py:511-544):
 *   dfd_kv_gather_patches    out[l, f*S + j, :] = src[l, f, index[l, j], :]  (+ pos[f % T]), K and V of all layers in one launch
 * Added beside the C ABI of dfdclip.h WITHOUT a new DFD_ABI_VERSION (still 17): no other header changed.  A library built
 * before it lacks the symbols, which the loader reports by name.  Conventions (device pointers, `stream`, return codes,
 * dfd_last_error) are dfdclip.h's.  The Python binding lists the entry points in capi.KVGATHER_SIGNATURES;
 * tests/test_kvgather_cpu.py checks header and table against each other, tests/test_hip_kvgather.py the kernel bit for bit
 * against `detector.gather_reference` on the same operands.
 *
 * Arithmetic.  Without `pos` the kept rows are copied, bit for bit.  With `pos` (f32) the entry is FIRST rounded to the tensor
 * type, then out = round(float(src) + float(round_to_dtype(pos[f % T, c]))): one add in f32 and one rounding (bf16: to nearest
 * even), which is what `src + pos.to(src.dtype)` computes in torch. */
#ifndef DFDCLIP_KVGATHER_H
#define DFDCLIP_KVGATHER_H

#include <stdint.h>

#include "dfdclip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Gather the kept patch rows of K and V.
 *   k, v       the sources, one element type; row (l, f, p) of either starts at base + l*stride_layer + f*stride_frame +
 *              p*stride_patch ELEMENTS (k and v share the strides) and holds D consecutive elements.  For the in-place q|k|v
 *              buffer [L, N, tokens, 3D] these are the views buf[:, :, 1:, D:2D] and buf[:, :, 1:, 2D:] with strides
 *              (N*tokens*3D, tokens*3D, 3D); for a contiguous export [L, N*P, D] they are (N*P*D, P*D, D).
 *   dtype      DFD_F32 or DFD_BF16: the type of k, v, k_out and v_out
 *   index      device int32 [L, S]: the kept patch positions of each tapped layer, in output order (unsorted and repeated
 *              entries are fine).  An entry outside [0, P) is clamped to it in the kernel: no address outside the named rows
 *              is ever formed.
 *   pos        device f32 [T, D], row stride D, or NULL
 *   k_out, v_out   [L, frames*S, D] contiguous, rows ordered (frame, kept position); must not overlap the sources
 *   L layers, `frames` frames per layer (clips * T), P patch rows per frame, S kept rows per frame, D elements per row.
 * One streaming launch, no workspace, no atomics, no LDS.  Every output element is written exactly once; nothing outside
 * the outputs is written and no source byte outside the rows that `index` names is read.  All offsets are 64-bit.  Two
 * forms of one arithmetic, bit for bit the same results:
 *   16-byte    a lane moves 16 bytes (8 bf16 / 4 f32) of a K row and of the V row beside it: taken when D, the three strides
 *              and k, v, k_out, v_out (and pos, when given) are all multiples of 16 bytes;
 *   by element everything else.
 * The source loads follow the DFD_STREAM_DECODER_KV bit of dfd_stream_policy_set (dfdclip_hooks.h): they are read once.  The
 * stores are plain: the decoder or the adapter reads them next.
 * L == 0, frames == 0 or S == 0 is a successful no-op.  Refused with DFD_ERR_INVALID_ARG and a message, without a launch: a
 * null pointer (pos may be NULL), any other dtype, S > P, a negative size, D <= 0 where there are rows, T <= 0,
 * frames % T != 0, stride_patch < D, a negative stride, L > 65535, frames * S >= 2^31 or D >= 2^30. */
int dfd_kv_gather_patches(const void* k, const void* v, int dtype, int64_t stride_layer, int64_t stride_frame, int64_t stride_patch,
                          const int32_t* index, const float* pos, void* k_out, void* v_out, int L, int64_t frames, int T, int P, int S, int D,
                          void* stream);

/* Which form the last successful dfd_kv_gather_patches of this thread launched: DFD_KVGATHER_VEC16 or DFD_KVGATHER_ELEMENT (0:
 * none yet, or the last call was a no-op).  For tests. */
#define DFD_KVGATHER_VEC16 1
#define DFD_KVGATHER_ELEMENT 2
int dfd_kv_gather_last_path(void);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_KVGATHER_H */
