/* Test and measurement hooks of libdfdclip_hip.so that are NOT part of the drop-in C ABI of dfdclip.h: they move no
 * device memory, select among kernels whose results the suite compares, and may change without a new DFD_ABI_VERSION.
 * The library exports them; the Python binding lists them in capi.HOOK_SIGNATURES. */
#ifndef DFDCLIP_HOOKS_H
#define DFDCLIP_HOOKS_H

#ifdef __cplusplus
extern "C" {
#endif

/* Which kernel dfd_attention_fwd picks.  0 (default) = as documented in dfdclip.h; 1 = the rows kernel (f32, and bf16
 * where no MFMA kernel serves the shape) stages K and V in chunks of 16 keys whatever the token count — the form it
 * otherwise takes only where K and V of a head exceed 160 KiB of LDS, bit-identical to the whole-head form; 2 = skip
 * the streaming bf16 MFMA kernel (attention_mfma_any.hip), so that the rows kernel serves the token counts outside the
 * 193..224 and 257..288 windows as it did before that kernel existed.  Per thread; returns the previous value. */
int dfd_attention_set_variant(int variant);

#ifdef __cplusplus
}
#endif
#endif
