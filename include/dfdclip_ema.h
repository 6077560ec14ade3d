/* dfdclip_ema.h — the EMA-teacher update for libdfdclip_hip.so: the trainer's teacher mode keeps a copy of the model whose
 * parameters follow the student's as an exponential moving average (the reference's src/trainer.py:179-185):
 *   dfd_ema_step    t = (1 - r) t + r s over every (teacher, student) parameter pair of a table, in one launch
 * Added beside the C ABI of dfdclip.h WITHOUT a new DFD_ABI_VERSION (still 17): no other header changed.  A library built
 * before it lacks the symbol, which the loader reports by name.  Conventions (device pointers, `stream`, return codes,
 * dfd_last_error) are dfdclip.h's.  The Python binding lists the entry point in capi.EMA_SIGNATURES; tests/test_ema_cpu.py
 * checks header and table against each other, tests/test_hip_ema.py the kernel bit for bit against the torch expression on
 * the same device.
 *
 * Arithmetic, per element, as torch evaluates `(1 - r) * t + r * s` on f32 tensors: both products are rounded to f32, then
 * their sum is — t = fadd_rn(fmul_rn(keep, t), fmul_rn(take, s)), never contracted into a fused multiply-add.  `keep` and
 * `take` are what torch casts its Python scalars to: keep = (float)(1.0 - r) and take = (float)r, formed from the double r
 * by the caller.  Non-finite elements follow IEEE: NaN stays NaN, inf - inf gives NaN, 0 * inf gives NaN. */
#ifndef DFDCLIP_EMA_H
#define DFDCLIP_EMA_H

#include <stdint.h>

#include "dfdclip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Blend every entry of the table.
 *   table_dev     DEVICE array of n dfd_sgd_param (dfdclip.h), laid out and dealt to workgroups exactly as for dfd_sgd_step:
 *                 `p` the teacher's parameter (read and written), `g` the student's (read only), `buf` unused and NULL,
 *                 `mirror` the [cols, rows] transposed copy of a [rows, cols] teacher weight, rewritten with the new values
 *                 through a 32 x 32 LDS tile by the same launch, or NULL (a flat run of `numel` elements, 1,024 per
 *                 workgroup); `first_block` of entry i = sum of dfd_sgd_blocks(...) of the entries before it
 *   total_blocks  the sum of dfd_sgd_blocks(...) over all entries: the grid
 *   keep, take    the two f32 factors (above)
 * Nothing but the `p` (and `mirror`) ranges of the entries is written.  `p` and `g` of an entry must not be the same
 * tensor: that is the caller's to check, who owns the table (a self-blend is not the identity in f32: (1 - r) x + r x != x
 * for about one element in six at r = 0.999).
 * The loads and stores follow the DFD_STREAM_OPTIMIZER bit of dfd_stream_policy_set (dfdclip_hooks.h): every byte is touched
 * once.  Both settings give the same bits.
 * Refused with DFD_ERR_INVALID_ARG and a message, without a launch: a null or empty table (n <= 0), total_blocks outside
 * [1, 2^31), a non-finite keep or take. */
int dfd_ema_step(const dfd_sgd_param* table_dev, int n, int64_t total_blocks, float keep, float take, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_EMA_H */
