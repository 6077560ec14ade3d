/* dfdclip_swiglu.h — the gate of a SwiGLU feed-forward for libdfdclip_hip.so: what DINOv2 ViT-g/14 runs between its `w12`
 * and `w3` Linears (the reference's dinov2/layers/swiglu_ffn.py, SwiGLUFFN.forward):
 *   dfd_swiglu_fwd    hidden[r, j] = silu(x12[r, j]) * x12[r, H + j]
 * Added beside the C ABI of dfdclip.h WITHOUT a new DFD_ABI_VERSION (still 17): no other header changed.  A library built
 * before it lacks the symbols, which the loader reports by name.  Conventions (device pointers, `stream`, return codes,
 * dfd_last_error) are dfdclip.h's.  The Python binding lists the entry points in capi.SWIGLU_SIGNATURES;
 * tests/test_dinov2_family_cpu.py checks header and table against each other, tests/test_hip_swiglu.py the kernel against
 * float64 on the same operands.
 *
 * Arithmetic.  Both operands are widened to f32; silu(x) = x / (1 + exp(-x)), with exp through the hardware's exp2 and the
 * quotient through its reciprocal (1 ulp each; the relative error of the exponential is about |x| * 2^-24); the product is
 * rounded ONCE to the output type (bf16: round to nearest even).  Every finite input gives a finite result: for x1 -> -inf
 * the exponential overflows to +inf and the result is +-0, never NaN; for x1 -> +inf it is x1 * x2.  Results below the
 * smallest normal f32 may be flushed to zero.  There is no backward pass: the tower that uses it is frozen. */
#ifndef DFDCLIP_SWIGLU_H
#define DFDCLIP_SWIGLU_H

#include <stdint.h>

#include "dfdclip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hidden = silu(x12[:, :H]) * x12[:, H:].
 *   x12      [rows, 2H], row stride ldx >= 2H elements; read exactly once
 *   hidden   [rows, H], row stride ldh >= H elements; must not overlap x12
 *   dtype    DFD_F32 or DFD_BF16: the type of BOTH tensors
 * One streaming launch, no workspace, no atomics, no LDS; every element of `hidden` is written exactly once and nothing
 * between the rows (columns H..ldh) is touched.  Two forms of one arithmetic, bit for bit the same results:
 *   16-byte    a lane loads 16 bytes of each half and stores 16 bytes (8 bf16 / 4 f32 gates): taken when H % 8 == 0 (bf16) /
 *              H % 4 == 0 (f32) and x12, hidden, ldx and ldh are all multiples of 16 bytes;
 *   by element everything else (any H, any alignment).
 * The loads of x12 follow the DFD_STREAM_ENCODER_ROWS bit of dfd_stream_policy_set (dfdclip_hooks.h).
 * rows < 2^31, H < 2^30.  rows == 0 or H == 0 is a successful no-op.  Refused with DFD_ERR_INVALID_ARG and a message, without
 * a launch: a null pointer, ldx < 2H, ldh < H, negative sizes, any other dtype. */
int dfd_swiglu_fwd(const void* x12, int64_t ldx, void* hidden, int64_t ldh, int dtype, int64_t rows, int H, void* stream);

/* Which form the last successful dfd_swiglu_fwd of this thread launched: DFD_SWIGLU_VEC16 or DFD_SWIGLU_ELEMENT (0: none yet, or
 * the last call was a no-op).  For tests. */
#define DFD_SWIGLU_VEC16 1
#define DFD_SWIGLU_ELEMENT 2
int dfd_swiglu_last_path(void);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_SWIGLU_H */
