/* dfdclip_ext.h — entry points of libdfdclip_hip.so added to the C ABI of dfdclip.h after DFD_ABI_VERSION 17 WITHOUT a new
 * version number: nothing in dfdclip.h changed (no signature, no struct layout, no enum value), and two tests pin 17
 * (tests/test_anytok_cpu.py, tests/test_adapter_structs_cpu.py).  A library built before them lacks the symbols, which the
 * loader reports by name.  Conventions (device pointers, `stream`, return codes, dfd_last_error) are dfdclip.h's.
 *
 * They live in a header of their own because the coverage rule of dfdclip.h — every function there has a guard-band test in
 * tests/test_hip_guarded.py — is checked against that one module; the functions here are covered by
 * tests/test_hip_guarded_dual.py under the same rule (tests/test_fp8_policy_cpu.py checks it).  The Python binding lists
 * them in capi.EXT_SIGNATURES. */
#ifndef DFDCLIP_EXT_H
#define DFDCLIP_EXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Dual-output forms of dfd_layernorm / dfd_layernorm2 / dfd_add_layernorm: ONE pass over the rows writes
 * y16 = bf16(LayerNorm(..)) (row stride ldy16) and y8 = e4m3(LayerNorm(..) * y8_inv_scale), saturated at +-448 (row stride
 * ldy8), from the same f32 values: each is bit-identical to what the single-output call writes for that type.  A layer of
 * the fp8 encoder whose K and V thirds stay on bf16 operands while its Q third runs on e4m3 reads both
 * (dfd-clip_amd/encoder.py, `set_fp8_policy`); the second output costs 1 byte per element instead of another pass over the
 * f32 rows.  Restrictions of the single-output twin (cols % 4 == 0; cols <= 4096 for dfd_layernorm_dual, <= 2048 for the
 * other two); y16 8-byte and y8 4-byte aligned, ldy16 % 4 == ldy8 % 4 == 0, y8_inv_scale > 0; neither output may alias x, a
 * delta or the other output. */
int dfd_layernorm_dual(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y16, int64_t ldy16, void* y8,
                       int64_t ldy8, int64_t rows, int cols, float eps, float y8_inv_scale, void* stream);
int dfd_layernorm2_dual(float* x, int64_t ldx, const float* gamma_a, const float* beta_a, const float* gamma_b, const float* beta_b,
                        void* y16, int64_t ldy16, void* y8, int64_t ldy8, int64_t rows, int cols, float eps, float y8_inv_scale,
                        void* stream);
int dfd_add_layernorm_dual(float* x, int64_t ldx, const void* delta, const void* delta2, int64_t ldd, int delta_dtype, int store_x,
                           const float* gamma, const float* beta, void* y16, int64_t ldy16, void* y8, int64_t ldy8, int64_t rows,
                           int cols, float eps, float y8_inv_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_EXT_H */
