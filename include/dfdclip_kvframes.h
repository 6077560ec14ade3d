/* dfdclip_kvframes.h — the frame mover of the streaming path for libdfdclip_hip.so (dfd_clip_amd/stream.py): whole frames of
 * K and V of every tapped layer, with a frame table on either side, in one launch:
 *   dfd_kv_move_frames    k_out[l, dst_frame[i], p, :] = k[l, src_frame[i], p, :]   (the same for v)
 * Added beside the C ABI of dfdclip.h WITHOUT a new DFD_ABI_VERSION (still 17): no other header changed.  A library built
 * before it lacks the symbols, which the loader reports by name.  Conventions (device pointers, `stream`, return codes,
 * dfd_last_error) are dfdclip.h's.  The Python binding lists the entry points in capi.KVFRAMES_SIGNATURES;
 * tests/test_stream_cpu.py checks header and table against each other, tests/test_hip_kvframes.py the kernel bit for bit
 * against `stream.move_reference` on the same operands.
 *
 * Arithmetic.  None: bits are copied. */
#ifndef DFDCLIP_KVFRAMES_H
#define DFDCLIP_KVFRAMES_H

#include <stdint.h>

#include "dfdclip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `flags` of dfd_kv_move_frames: the source is read once (the ingest of a frame store), so its loads follow the
 * DFD_STREAM_DECODER_KV bit of dfd_stream_policy_set (dfdclip_hooks.h).  Without it the loads are plain: a window gather reads
 * a stored frame once per window that holds it. */
#define DFD_KVFRAMES_SRC_ONCE 1

/* Move n frames of K and V.
 *   k, v       the sources, one element type; row (l, f, p) of either starts at base + l*src_stride_layer + f*src_stride_frame +
 *              p*src_stride_patch ELEMENTS (k and v share the strides) and holds D consecutive elements.  For the in-place
 *              q|k|v buffer [L, N, tokens, 3D] these are the views buf[:, :, 1:, D:2D] and buf[:, :, 1:, 2D:] with strides
 *              (N*tokens*3D, tokens*3D, 3D); for a dense store [L, C, P, D] they are (C*P*D, P*D, D).
 *   k_out, v_out   the destinations, addressed the same way with the dst strides (shared by both); must not overlap the sources
 *   dtype      DFD_F32 or DFD_BF16: the type of all four tensors
 *   src_frame, dst_frame   device int32 [n], or NULL for the identity i.  An entry outside [0, src_frames) or [0, dst_frames)
 *              is clamped to it in the kernel before any address is formed.  Distinct dst_frame entries are the caller's
 *              duty (two moves into one frame race); the kernel does not check.  Repeated src_frame entries are fine.
 *   L layers, n frames to move, src_frames / dst_frames frames per layer on either side, P patch rows per frame, D elements
 *   per row.
 * One streaming launch, no workspace, no atomics, no LDS.  Nothing outside the named destination rows is written (the
 * elements between D and dst_stride_patch included) and no source byte outside the named rows is read.  All offsets are
 * 64-bit: a layer stride above 2^31 elements is fine.  Two forms, bit for bit the same results:
 *   16-byte    a lane moves 16 bytes (8 bf16 / 4 f32) of a K row and of the V row beside it: taken when D, all six strides
 *              and k, v, k_out, v_out are multiples of 16 bytes;
 *   by element everything else.
 * The stores are plain: the decoder or the adapter reads them next.
 * L == 0, n == 0 or P == 0 is a successful no-op.  Refused with DFD_ERR_INVALID_ARG and a message, without a launch: a null
 * k / v / k_out / v_out, any other dtype, a negative size or stride, a patch stride < D, L > 65535, n * P >= 2^31,
 * D >= 2^30, D <= 0 or src_frames <= 0 or dst_frames <= 0 where there are rows, an unknown flag bit. */
int dfd_kv_move_frames(const void* k, const void* v, void* k_out, void* v_out, int dtype,
                       int64_t src_stride_layer, int64_t src_stride_frame, int64_t src_stride_patch,
                       int64_t dst_stride_layer, int64_t dst_stride_frame, int64_t dst_stride_patch,
                       const int32_t* src_frame, const int32_t* dst_frame,
                       int L, int64_t n, int src_frames, int dst_frames, int P, int D,
                       int flags, void* stream);

/* Which form the last successful dfd_kv_move_frames of this thread launched: DFD_KVFRAMES_VEC16 or DFD_KVFRAMES_ELEMENT (0:
 * none yet, or the last call was a no-op).  For tests. */
#define DFD_KVFRAMES_VEC16 1
#define DFD_KVFRAMES_ELEMENT 2
int dfd_kv_move_last_path(void);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_KVFRAMES_H */
