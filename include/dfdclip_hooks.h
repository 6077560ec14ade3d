/* Test and measurement hooks of libdfdclip_hip.so that are NOT part of the drop-in C ABI of dfdclip.h: they move no
 * device memory, select among kernels whose results the suite compares, and may change without a new DFD_ABI_VERSION.
 * The library exports them; the Python binding lists them in capi.HOOK_SIGNATURES. */
#ifndef DFDCLIP_HOOKS_H
#define DFDCLIP_HOOKS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Which kernel dfd_attention_fwd picks.  0 (default) = as documented in dfdclip.h; 1 = the rows kernel (f32, and bf16
 * where no MFMA kernel serves the shape) stages K and V in chunks of 16 keys whatever the token count — the form it
 * otherwise takes only where K and V of a head exceed 160 KiB of LDS, bit-identical to the whole-head form; 2 = skip
 * the streaming bf16 MFMA kernel (attention_mfma_any.hip), so that the rows kernel serves the token counts outside the
 * 193..224 and 257..288 windows as it did before that kernel existed.  Per thread; returns the previous value. */
int dfd_attention_set_variant(int variant);

/* The c_fc -> c_proj pair of the encoder's MLP (DFD_GEMM_C_BLOCKED / DFD_GEMM_A_BLOCKED).  0 (default) = the pair keeps
 * the intermediate fragment-blocked where dfd_gemm_pair_plan says so; 1 = row-major everywhere: the plan answers 0 and a
 * call that carries one of the bits runs on the same kernel with a row-major C / A (the bits then only waive the
 * M >= 1024 rule) — the A/B switch; 2 = the plan also answers 1 below 1024 rows (tests: two frames are enough to cross a
 * ragged panel).  Per thread; returns the previous value. */
int dfd_gemm_pair_set_variant(int variant);
/* 1 = an MLP pair u[M, H] = act(h[M, D] . Wfc^T), delta[M, D] = u . Wproj^T on bf16 operands with dense rows runs both
 * halves on the ping-pong kernel and keeps u fragment-blocked (the caller then sets the two bits and passes the permuted
 * c_fc weights); 0 = the row-major pair.  The one place that decides it. */
int dfd_gemm_pair_plan(int64_t M, int D, int H);
/* The number of this thread's dfd_gemm calls so far that wrote or read a fragment-blocked matrix (served with
 * DFD_GEMM_C_BLOCKED or DFD_GEMM_A_BLOCKED in force; not the calls variant 1 turned row-major).  For tests. */
int64_t dfd_gemm_pair_launches(void);

/* Which kernels served this thread's last successful dfd_gemm_at_b: 128 or 256 = the transposing-LDS-read kernel of
 * gemm_tn.hip at that tile width (bf16, both extents multiples of 128 resp. 256, ld % 8 == 0, 16-byte aligned bases);
 * 1 = transposes into the workspace + the general split-K kernel (everything else); 0 = no call yet.  What
 * dfd_gemm_last_path is to dfd_gemm. */
int dfd_gemm_at_b_last_path(void);

/* The cache policy of the kernels that touch every byte once.  One bit per family; a set bit makes that family's loads
 * and stores of its read-once (write-once) stream non-temporal, so that they do not evict what the persistent GEMMs of
 * another stream keep in L2.  Results are bit-identical either way (tests/test_hip_stream_policy.py).  Process-wide
 * (the backward pass launches from another thread than the forward); read at launch, so a captured graph keeps what was
 * set at capture.  `set` returns the previous mask; DFD_STREAM_DEFAULT is what the library starts with. */
enum {
  DFD_STREAM_DECODER_KV = 1,      /* K / V loads of dfd_decoder_attn_fwd and dfd_decoder_attn_bwd */
  DFD_STREAM_DECODER_WEIGHTS = 2, /* weight loads of dfd_linear_rows / dfd_linear_rows_t, dW stores of dfd_linear_rows_bwd_weight */
  DFD_STREAM_OPTIMIZER = 4,       /* dfd_sgd_step: gradient, state and parameter loads; state, parameter and mirror stores */
  DFD_STREAM_ENCODER_ROWS = 8,    /* the LayerNorm family's f32 x / delta loads and f32 x store; dfd_patchify's frame loads */
  DFD_STREAM_ALL = 15
};
/* DECODER_KV | ENCODER_ROWS: the families that passed the rule of DESIGN.md section 7.1b */
#define DFD_STREAM_DEFAULT 9
unsigned dfd_stream_policy_set(unsigned mask);
unsigned dfd_stream_policy_get(void);

#ifdef __cplusplus
}
#endif
#endif
