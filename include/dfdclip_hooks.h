/* Test and measurement hooks of libdfdclip_hip.so that are NOT part of the drop-in C ABI of dfdclip.h: they move no
 * device memory, select among kernels whose results the suite compares, and may change without a new DFD_ABI_VERSION.
 * The library exports them; the Python binding lists them in capi.HOOK_SIGNATURES. */
#ifndef DFDCLIP_HOOKS_H
#define DFDCLIP_HOOKS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The kernels behind dfd_attention_fwd and the rule that picks one (attn_plan in csrc/attention_common.hpp is the only
 * code that knows it).  items = n_frames * heads, esz = bytes per element, n_cu = compute units of the device (256 where
 * it cannot be queried), the two extents are the bytes a persistent kernel addresses with 32-bit offsets:
 *   qkv_bytes = (n_frames*tokens - 1) * ld_qkv * 2 + 3*heads*128,   out_bytes = (n_frames*tokens - 1) * ld_out * 2 + heads*128.
 * The first row that matches wins; bf16 unless it says f32:
 *   f32, or tokens <= 32                                                          -> rows (below)
 *   193..224 tokens, items >= 512, tokens <= 208, both extents <= 0xfffffff0,
 *     (n_cu & ~7) >= 8                                   -> PERSIST7_SHORT (tokens <= 200) or PERSIST7:
 *                                                           grid n_cu & ~7, block 512, LDS 512*tokens + 57,344
 *   193..224 tokens otherwise                            -> ITEM7: grid items, block 256, LDS 57,856
 *   257 tokens, items >= 512, both extents fit, (n_cu & ~7) >= 8
 *                                                        -> XROW: grid n_cu & ~7, block 512, LDS 150,528
 *   257..288 tokens otherwise                            -> ITEM9: grid items, block 256, LDS 74,240
 *   33 tokens and up, variant != 2, items * ceil(tokens / 128) <= 2^31 - 1
 *                                                        -> STREAM: that grid, block 256, no dynamic LDS
 *   everything else                                      -> rows
 * rows: grid items, block 256; chunk = 16 keys under variant 1, else 65,536 / (128*esz) keys where K and V of a head
 * (2*tokens*64*esz bytes) exceed 160 KiB (f32 above 320 tokens, bf16 above 640), else 0.  chunk > 0 -> ROWS_CHUNKED with
 * LDS 2*chunk*64*esz, else ROWS with LDS 2*tokens*64*esz.  A call whose items exceed 2^31 - 1 on a path whose grid is
 * `items` (rows, ITEM7, ITEM9) is refused. */
enum {
  DFD_ATTN_ROWS = 1,           /* attention.hip: K and V of a head in LDS, one query row per thread */
  DFD_ATTN_ROWS_CHUNKED = 2,   /* attention.hip: the same arithmetic, K and V staged in key chunks */
  DFD_ATTN_ITEM7 = 3,          /* attention_mfma.hip: one workgroup per item, 7 key blocks */
  DFD_ATTN_ITEM9 = 4,          /* attention_mfma.hip: one workgroup per item, 9 key blocks */
  DFD_ATTN_PERSIST7_SHORT = 5, /* attention_mfma.hip: persistent, at most 8 keys in the last block */
  DFD_ATTN_PERSIST7 = 6,       /* attention_mfma.hip: persistent */
  DFD_ATTN_XROW = 7,           /* attention_mfma_xrow.hip: persistent, 257 tokens */
  DFD_ATTN_STREAM = 8          /* attention_mfma_any.hip: streaming, any token count */
};
typedef struct {
  int32_t path;         /* DFD_ATTN_* */
  uint32_t grid, block; /* workgroups and threads per workgroup */
  int32_t chunk;        /* keys per staging chunk of DFD_ATTN_ROWS_CHUNKED, else 0 */
  uint64_t lds;         /* dynamic LDS bytes of the launch */
} dfd_attention_plan_t;

/* The path (DFD_ATTN_*) of this thread's last successful dfd_attention_fwd that launched a kernel; 0 = no call yet. */
int dfd_attention_last_path(void);
/* What dfd_attention_fwd would do with this shape under the thread's current variant: returns the path and fills *out
 * (may be NULL), or returns -1 with dfd_last_error() for what dfd_attention_fwd refuses.  No pointer is involved and,
 * with n_cu > 0, no device (n_cu <= 0: the current device's count). */
int dfd_attention_plan(int dtype, int n_frames, int tokens, int heads, int64_t ld_qkv, int64_t ld_out, int n_cu,
                       dfd_attention_plan_t* out);

/* Changes the selection above.  0 (default) = the table; 1 = the rows kernel (f32, and bf16 where no MFMA kernel serves
 * the shape) stages K and V in chunks of 16 keys whatever the token count — the form it otherwise takes only where K
 * and V of a head exceed 160 KiB of LDS, bit-identical to the whole-head form; 2 = skip the streaming bf16 MFMA kernel
 * (attention_mfma_any.hip), so that the rows kernel serves the token counts outside the 193..224 and 257..288 windows
 * as it did before that kernel existed.  Per thread; returns the previous value. */
int dfd_attention_set_variant(int variant);

/* The kernels behind dfd_gemm and dfd_gemm_fp8 and the rule that picks one (gemm_plan in csrc/gemm_plan.hpp is the only
 * code that knows it).  A K step is 128 bytes of an operand row: 64 bf16 or 128 e4m3 elements; steps = K / that.  "aligned":
 * 16 bytes.  The first row that matches wins:
 *   f32 operands                                                                   -> GENERAL (below)
 *   PINGPONG, unless dfd_gemm_set_variant(1): bf16 or e4m3 operands; C bf16 (e4m3 operands, no QKV_EXPORT: or e4m3);
 *     M >= 1024 (one half of a c_fc -> c_proj pair: any M); N % 256 == 0; steps even and >= 6 (RESIDUAL_POS: or 4);
 *     ldw a multiple of 128 bytes, lda and ldc of 16; A, W, C, bias (e4m3: and col_scale) aligned; the bytes of A, W and C
 *     (M rounded up to 16 in a pair) each <= 0xfffffff0; ceil(M / 224) * N / 256 <= 0x3fffffff; M < 2^31;
 *     BIAS, BIAS_QUICKGELU, BIAS_GELU, QKV_EXPORT, and for bf16 RESIDUAL_POS;
 *     DFD_GEMM_C_BLOCKED: bf16, ldc % 64 == 0, BIAS_QUICKGELU / BIAS_GELU; DFD_GEMM_A_BLOCKED: bf16, lda % 64 == 0, BIAS;
 *     QKV_EXPORT with export buffers (without them it is BIAS here): the column block N / (3 - qkv_first) a multiple of
 *     256, pos aligned, the export's bytes <= 0xfffffff0; RESIDUAL_POS: M * (N / 8) < 2^32, pos and residual aligned
 *   PERSISTENT: the same rules with steps >= 2 and ldw a multiple of 16 bytes; BIAS, BIAS_QUICKGELU, QKV_EXPORT, and for
 *     e4m3 BIAS_GELU; no blocked layout
 *   a call with DFD_GEMM_C_BLOCKED / _A_BLOCKED that PINGPONG does not serve, and an e4m3 call neither serves -> refused
 *   TILE: bf16 operands; M >= 1024; N % 256 == 0; K % 64 == 0, K >= 128; lda % 8 == ldw % 8 == ldc % 4 == 0; C and bias
 *     aligned; ceil(M / 256) * N / 256 <= 2^31 - 1; M < 2^31; BIAS, BIAS_QUICKGELU, QKV_EXPORT (column block a multiple of
 *     256, pos aligned) with either C; BIAS_RESIDUAL and PATCH_EMBED (pos, cls aligned) with f32 C; RESIDUAL_POS with bf16
 *     C, ldc % 8 == 0, pos and residual aligned
 *   GENERAL: everything else dfd_gemm accepts (BIAS_RESIDUAL, PATCH_EMBED: f32 C, else refused)
 * Launches: GENERAL grid (ceil(N / 128), ceil(M / 128)), block 256; TILE grid ceil(M / 256) * N / 256, block 512; the
 * persistent two: block 512, tiles of tile_rows x 256, grid = min(tiles, CUs), CUs = max(n_cu - spare_cus, n_cu / 2).
 * tile_rows: e4m3 256; RESIDUAL_POS 224; DFD_GEMM_TILE_BLOCKS 7 / 8 forced; else 224 where 0.97 * rounds(224) <
 * rounds(256), rounds(r) = ceil(ceil(M / r) * N / 256 / CUs).  DFD_GEMM_SPARE_IF_FREE (PINGPONG only): CUs = n_cu where the
 * cheaper height's cost on n_cu is below that on CUs.  dynamic: PINGPONG, bf16, steps >= 6, dfd_gemm_set_variant(3). */
enum { DFD_GEMM_GENERAL = 1, /* gemm.hip: 128x128 tiles, any shape */
       DFD_GEMM_TILE = 2,    /* gemm256.hip: one workgroup per 256x256 tile */
       DFD_GEMM_PERSISTENT = 3, /* gemm256p.hip: persistent, every K depth from two steps */
       DFD_GEMM_PINGPONG = 4 /* gemm256e.hip: persistent, ping-pong K loop */ };
/* one bit per pointer of a call, for dfd_gemm_plan's `has` and `misaligned` */
enum { DFD_GEMM_PTR_A = 1, DFD_GEMM_PTR_W = 2, DFD_GEMM_PTR_C = 4, DFD_GEMM_PTR_BIAS = 8, DFD_GEMM_PTR_POS = 16, DFD_GEMM_PTR_CLS = 32,
       DFD_GEMM_PTR_RESIDUAL = 64, DFD_GEMM_PTR_COL_SCALE = 128, DFD_GEMM_PTR_EXPORT = 256 /* k_export and v_export */ };
typedef struct {
  int32_t kernel;             /* DFD_GEMM_* */
  int32_t epilogue;           /* of the instantiation: QKV_EXPORT without export buffers is BIAS on the persistent kernels */
  int32_t tile_rows, tiles_m; /* tile height and row panels */
  int64_t ntiles;
  uint32_t grid, grid_y, block;
  int32_t c_blocked, a_blocked; /* the layout flags in force (dfd_gemm_pair_set_variant(1) clears them) */
  int32_t dynamic;              /* 1 = the dynamic tile hand-out may be prepared */
} dfd_gemm_plan_t;

/* The kernel (DFD_GEMM_*) of this thread's last successful dfd_gemm or dfd_gemm_fp8 that launched one; 0 = none yet.
 * dfd_gemm_last_path (dfdclip.h) reports dfd_gemm's share of the same record as 128 / 256 / 257. */
int dfd_gemm_last_kernel(void);
/* What dfd_gemm (ab_dtype DFD_F32 / DFD_BF16) or dfd_gemm_fp8 (DFD_FP8) would do with a call under the thread's current
 * variants: returns the kernel (0 for M == 0: nothing is launched) and fills *out (may be NULL), or returns -1 with
 * dfd_last_error() in the words of the entry point.  flags: dfd_gemm_extra.flags; has: which of DFD_GEMM_PTR_EXPORT, _POS,
 * _RESIDUAL the call carries (the others are taken as present); misaligned: the pointers that are not 16-byte aligned, 0 =
 * none.  No pointer is involved and, with n_cu > 0, no device (n_cu <= 0: the current device's count). */
int dfd_gemm_plan(int ab_dtype, int c_dtype, int epilogue, int64_t M, int N, int K, int64_t lda, int64_t ldw, int64_t ldc,
                  uint32_t flags, int tokens, int frames_per_clip, int qkv_first, unsigned has, unsigned misaligned, int n_cu,
                  dfd_gemm_plan_t* out);

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

/* The kernels behind dfd_adapter_norm_gelu and the group pass of dfd_adapter_norm_gelu_bwd, and the rule that picks one
 * (adp_plan in csrc/adapter.hip is the only code that knows it).  groups = frames (mode 1) or frames * patches (modes 0
 * and 2); group = patches * x (mode 1) or x; "aligned": a, the output, dy (backward), weight and bias at 16 bytes.
 *   mode 1, aligned, group % 8 == 0, group <= 57,344 (7 chunks x 1024 threads x 8) -> JOINT_REG: grid groups, block 1024
 *   mode 1 otherwise                                                               -> JOINT:     grid groups, block 1024
 *   modes 0 and 2, aligned, x == 256                              -> ROW256: grid ceil(groups / 4), block 256
 *   modes 0 and 2 otherwise                                       -> ROW: forward grid ceil(groups / 4), block 256;
 *                                                                         backward grid groups, block 64
 * Backward then adds the affine gradients in slabs = min(ceil(262,144 / group), groups, 512) partial slabs of
 * groups_per_slab = ceil(groups / slabs) groups each (slabs past the last group add zeros) and one reduction.
 * A call whose patches * x reaches 2^31, or whose grid exceeds 2^31 - 1, is refused. */
enum { DFD_ADP_ROW256 = 1,    /* one wave per 256-wide row, four elements per lane */
       DFD_ADP_JOINT_REG = 2, /* one workgroup per frame, the slab held in registers */
       DFD_ADP_JOINT = 3,     /* one workgroup per frame, the slab read once per pass */
       DFD_ADP_ROW = 4        /* the strided row kernels, any x, any alignment */ };
typedef struct {
  int32_t path;                   /* DFD_ADP_*; 0 = forward with frames == 0: nothing is launched */
  uint32_t grid, block;           /* of the forward kernel, or of the backward's group pass */
  int32_t slabs, groups_per_slab; /* backward: the affine pass; forward: 0 */
} dfd_adapter_plan_t;

/* The path (DFD_ADP_*) of this thread's last successful dfd_adapter_norm_gelu or dfd_adapter_norm_gelu_bwd that launched
 * a kernel; 0 = no call yet. */
int dfd_adapter_norm_gelu_last_path(void);
/* What dfd_adapter_norm_gelu (backward == 0) or dfd_adapter_norm_gelu_bwd would do with this shape: returns the path and
 * fills *out (may be NULL), or returns -1 with dfd_last_error() in the words of that entry point.  misaligned != 0: one
 * of the pointers named above is not 16-byte aligned.  No pointer and no device is involved. */
int dfd_adapter_norm_gelu_plan(int frames, int patches, int x, int joint, int a_dtype, int dtype, int misaligned, int backward,
                               dfd_adapter_plan_t* out);

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
