// The host side of the four kernels behind dfd_gemm and dfd_gemm_fp8 — gemm128 (gemm.hip), gemm256 (gemm256.hip), gemm256p
// (gemm256p.hip), gemm256e (gemm256e.hip): which kernel serves a call and with which tiles (gemm_plan), the one launch
// helper, and the launcher each file exports.  gemm_plan is the only place that knows shape thresholds, K depths, leading-
// dimension and pointer alignment, 32-bit extents, which epilogue has which instantiation and the rules of the c_fc ->
// c_proj pair; its table is written out once, in include/dfdclip_hooks.h.  A new kernel or rule is a constant there, a row
// here, a case in one file's launcher and a row of the table in tests/test_abi_cpu.py.
#pragma once
#include "gemm_args.hpp"

#include "../../include/dfdclip_hooks.h"

// What the plan may know of a call's pointers: which are there, and which are not 16-byte aligned (DFD_GEMM_PTR_* bits).
struct GemmPtrs {
  unsigned present, misaligned;
};
inline GemmPtrs gemm_ptrs(const GemmArgs& a) {
  const void* const ptr[] = {a.A, a.W, a.C, a.bias, a.pos, a.cls, a.residual, a.col_scale, a.k_export};  // in DFD_GEMM_PTR_* order
  GemmPtrs p{0u, 0u};
  for (unsigned i = 0; i < sizeof(ptr) / sizeof(ptr[0]); ++i) {
    if (ptr[i] != nullptr) p.present |= 1u << i;
    if ((reinterpret_cast<uintptr_t>(ptr[i]) & 15) != 0) p.misaligned |= 1u << i;
  }
  return p;
}

struct TilePlan {
  int rows, tiles_m;  // tile height (persistent kernels: 224 / 256) and row panels
  int64_t ntiles;
  int grid;  // workgroups; persistent kernels: min(CUs left to this launch, tiles), 0: no device
};

struct GemmPlan {
  int kernel;    // DFD_GEMM_*, 0: no kernel (nothing to do, or `refused`)
  int epilogue;  // the instantiation's: QKV_EXPORT without export buffers is BIAS on the persistent kernels
  int c_blocked, a_blocked;  // the layout the ping-pong kernel writes / reads: the call's flags, unless dfd_gemm_pair_set_variant(1) clears them
  int dynamic;               // gemm256e.hip: the dynamic tile hand-out may be prepared
  TilePlan tiles;
  unsigned grid_y, block;  // grid = (tiles.grid, grid_y)
  const char* refused;     // kernel == 0: the rule that refused the call (of the last kernel that could have served it)
};

constexpr int GEMM_TILE_N = 256;  // output tile width of the three tuned kernels
constexpr int64_t GEMM_EXTENT_MAX = 0xfffffff0;  // buffer descriptors carry 32-bit byte offsets

// the epilogues each persistent family has an instantiation for
constexpr bool gemm_serves(int kernel, int epi, bool f8) {
  const bool both = epi == DFD_EPI_BIAS || epi == DFD_EPI_BIAS_QUICKGELU || epi == DFD_EPI_QKV_EXPORT;
  return kernel == DFD_GEMM_PINGPONG ? both || epi == DFD_EPI_BIAS_GELU || (!f8 && epi == DFD_EPI_RESIDUAL_POS) : both || (f8 && epi == DFD_EPI_BIAS_GELU);
}

// spare_if_free: `spare_cus` is a request, not an order — honoured where the rounds of tiles (at the best height allowed)
// stay the same.  force224: the epilogue only exists for 224-row tiles.
inline TilePlan plan_tiles(int64_t M, int N, int spare_cus, bool spare_if_free, int tile_rows, bool f8, bool force224, int n_cu) {
  const int tiles_n = N / GEMM_TILE_N;
  if (n_cu <= 0) return TilePlan{0, 0, 0, 0};
  int cus = n_cu - spare_cus;
  cus = cus < n_cu / 2 ? n_cu / 2 : cus;
  // tile height: the one with the least (rounds of tiles) x (cost of a tile).  A 224-row tile saves the MFMA and
  // epilogue work of 32 rows but stages as many bytes as a 256-row one, and the loop is bound by that staging:
  // measured on the four ViT-B/16 shapes it costs 0.97 of a full tile, so it wins only where it saves a whole
  // round (M = 94,560: N = 768 needs 5 rounds either way -> 224; N = 2304 / 3072: 15 vs 14, 20 vs 18 -> 256)
  auto cost = [&](int rows, int c) { return (double)((((M + rows - 1) / rows) * tiles_n + c - 1) / c) * (rows == 224 ? 0.97 : 1.0); };
  if (spare_cus > 0 && spare_if_free) {
    auto best = [&](int c) { return f8 ? cost(256, c) : force224 ? cost(224, c) : (cost(224, c) < cost(256, c) ? cost(224, c) : cost(256, c)); };
    if (best(cus) > best(n_cu)) cus = n_cu;
  }
  const bool use224 = !f8 && (force224 || tile_rows == 224 || (tile_rows == 0 && cost(224, cus) < cost(256, cus)));
  TilePlan p;
  p.rows = use224 ? 224 : 256;
  p.tiles_m = (int)((M + p.rows - 1) / p.rows);
  p.ntiles = (int64_t)p.tiles_m * tiles_n;
  p.grid = (int)(p.ntiles < cus ? p.ntiles : cus);
  return p;
}

// The rule by which persistent kernel `kernel` (DFD_GEMM_PINGPONG / _PERSISTENT) refuses the call, NULL where it serves it.
// cb / ab: the layout flags in force.
inline const char* gemm_persistent_refuses(int kernel, const GemmArgs& a, GemmPtrs p, bool f8, int c_dtype, int epi, int cb, int ab) {
  const bool pingpong = kernel == DFD_GEMM_PINGPONG, cf8 = c_dtype == DFD_FP8;
  const int esz = f8 ? 1 : 2, csz = cf8 ? 1 : 2, kshift = f8 ? 7 : 6;  // a K step is 128 bytes of every operand row: 2^kshift elements
  if (c_dtype != DFD_BF16 && !(f8 && cf8)) return "C must be bf16 (e4m3 operands: or e4m3)";
  if (f8 && (!(p.present & DFD_GEMM_PTR_COL_SCALE) || (p.misaligned & DFD_GEMM_PTR_COL_SCALE))) return "col_scale must be 16-byte aligned";
  if (a.N % GEMM_TILE_N != 0) return "N % 256 != 0";
  if ((a.K & ((1 << kshift) - 1)) != 0) return "a row of K is not a whole number of 128-byte steps";
  if (a.M < 1024 && !a.pair) return "M < 1024";  // (one half of a c_fc -> c_proj pair: any M)
  if ((a.lda * esz) % 16 != 0 || (a.ldw * esz) % 16 != 0 || (a.ldc * csz) % 16 != 0) return "lda, ldw and ldc must be 16-byte multiples";
  if (p.misaligned & (DFD_GEMM_PTR_A | DFD_GEMM_PTR_W | DFD_GEMM_PTR_C | DFD_GEMM_PTR_BIAS)) return "A, W, C and bias must be 16-byte aligned";
  const int64_t Mr = a.pair ? (a.M + 15) & ~(int64_t)15 : a.M;  // a blocked matrix keeps whole groups of 16 rows
  if (Mr * a.lda * esz > GEMM_EXTENT_MAX || (int64_t)a.N * a.ldw * esz > GEMM_EXTENT_MAX || Mr * a.ldc * csz > GEMM_EXTENT_MAX)
    return "A, W or C exceeds the 32-bit byte offsets of a buffer descriptor";
  if ((int64_t)((a.M + 223) / 224) * (a.N / GEMM_TILE_N) > 0x3fffffff || a.M >= ((int64_t)1 << 31)) return "too many tiles or rows";
  // the fragment-blocked layout (gemm_blocked.hpp): bf16, whole 64-channel K tiles in every row group
  if ((cb || ab) && (esz != 2 || csz != 2)) return "the fragment-blocked layout is bf16";
  if ((cb && a.ldc % 64 != 0) || (ab && a.lda % 64 != 0)) return "the leading dimension of a fragment-blocked matrix must be a multiple of 64";
  const int nk = a.K >> kshift;
  if (pingpong) {
    // the loop is unrolled in pairs of K tiles around a head of two and a tail of four (RESIDUAL_POS: also the short form, 4)
    if ((nk < 6 && !(epi == DFD_EPI_RESIDUAL_POS && nk == 4)) || (nk & 1)) return "the ping-pong K loop needs an even number of 128-byte steps, at least 6";
    if ((a.ldw * esz) % 128 != 0) return "ldw must be a multiple of 128 bytes";  // the second piece of a W unit is addressed as (first ^ 64) + 8 rows
  } else if (nk < 2) {
    return "K is less than two 128-byte steps";
  }
  if (!gemm_serves(kernel, epi, f8)) return "the kernel has no form for this epilogue";
  // blocked C: the MLP's activation epilogues write it; blocked A: the plain epilogue reads it (gemm256e.hip only)
  if ((cb || ab) && !pingpong) return "only the ping-pong kernel knows the fragment-blocked layout";
  if (cb && epi != DFD_EPI_BIAS_QUICKGELU && epi != DFD_EPI_BIAS_GELU) return "DFD_GEMM_C_BLOCKED needs BIAS_QUICKGELU or BIAS_GELU";
  if (ab && epi != DFD_EPI_BIAS) return "DFD_GEMM_A_BLOCKED needs BIAS";
  if (epi == DFD_EPI_QKV_EXPORT) {
    const int D = a.N / (3 - a.qkv_first);
    if (cf8) return "an e4m3 C has no QKV_EXPORT form";
    if (D % GEMM_TILE_N != 0) return "a q / k / v column block is not a multiple of 256";
    if (p.misaligned & DFD_GEMM_PTR_POS) return "pos must be 16-byte aligned";
    if ((p.present & DFD_GEMM_PTR_EXPORT) && (a.M / a.tokens) * (a.tokens - 1) * (int64_t)D * 2 > GEMM_EXTENT_MAX) return "the K / V export exceeds 32-bit byte offsets";
  }
  if (epi == DFD_EPI_RESIDUAL_POS) {
    if (a.tokens < 2 || a.M * (int64_t)(a.N >> 3) >= ((int64_t)1 << 32)) return "RESIDUAL_POS needs tokens and M * N / 8 < 2^32";
    if ((p.misaligned & (DFD_GEMM_PTR_POS | DFD_GEMM_PTR_RESIDUAL)) || ((p.present & DFD_GEMM_PTR_POS) && a.frames_per_clip < 1))
      return "pos and residual must be 16-byte aligned";
  }
  return nullptr;
}

// ... gemm256.hip (one workgroup per 256x256 tile; bf16 operands, bf16 or f32 C)
inline const char* gemm_tile_refuses(const GemmArgs& a, GemmPtrs p, int c_dtype, int epi) {
  if (a.N % GEMM_TILE_N != 0 || a.K % 64 != 0 || a.K < 128 || a.M < 1024) return "N % 256, K % 64, K >= 128, M >= 1024";
  if ((a.lda % 8) != 0 || (a.ldw % 8) != 0 || (a.ldc % 4) != 0) return "leading dimensions";
  if (p.misaligned & (DFD_GEMM_PTR_C | DFD_GEMM_PTR_BIAS)) return "C and bias must be 16-byte aligned";
  if ((int64_t)((a.M + 255) / 256) * (a.N / GEMM_TILE_N) > 0x7fffffff) return "too many tiles";
  if (a.M >= ((int64_t)1 << 31)) return "too many rows";  // the epilogues index rows with 32-bit arithmetic
  const bool bf = c_dtype == DFD_BF16;
  switch (epi) {
    case DFD_EPI_BIAS:
    case DFD_EPI_BIAS_QUICKGELU:
      return nullptr;
    case DFD_EPI_QKV_EXPORT:
      return (a.N / (3 - a.qkv_first)) % GEMM_TILE_N != 0 || (p.misaligned & DFD_GEMM_PTR_POS) ? "column blocks of 256, aligned pos" : nullptr;
    case DFD_EPI_BIAS_RESIDUAL:
      return bf ? "f32 C only" : nullptr;
    case DFD_EPI_RESIDUAL_POS:
      return !bf || (a.ldc % 8) != 0 || (p.misaligned & (DFD_GEMM_PTR_POS | DFD_GEMM_PTR_RESIDUAL)) ? "bf16 C, ldc % 8, aligned pos and residual" : nullptr;
    case DFD_EPI_PATCH_EMBED:
      return bf || (p.misaligned & (DFD_GEMM_PTR_POS | DFD_GEMM_PTR_CLS)) ? "f32 C, aligned pos and cls" : nullptr;
    default:
      return "no form for this epilogue";
  }
}

// ... gemm.hip's general kernel: any shape dfd_gemm accepts
inline const char* gemm_general_refuses(int c_dtype, int epi) {
  switch (epi) {
    case DFD_EPI_BIAS:
    case DFD_EPI_BIAS_QUICKGELU:
    case DFD_EPI_BIAS_GELU:
    case DFD_EPI_QKV_EXPORT:
    case DFD_EPI_RESIDUAL_POS:
      return nullptr;
    case DFD_EPI_BIAS_RESIDUAL:
    case DFD_EPI_PATCH_EMBED:
      return c_dtype == DFD_F32 ? nullptr : "the epilogue needs an f32 C";
    default:
      return "unknown epilogue";
  }
}

// The plan of a call that dfd_gemm (ab_dtype F32 / BF16) or dfd_gemm_fp8 (FP8) has accepted: the first kernel in the order
// ping-pong, persistent, tile, general that serves it.  f32 operands go straight to the general kernel; e4m3 operands have
// the two persistent kernels only; one half of a c_fc -> c_proj pair has the ping-pong kernel only; dfd_gemm_set_variant(1)
// skips the ping-pong kernel.  Reads numbers, never a pointer; no HIP call.
inline GemmPlan gemm_plan(const GemmArgs& a, GemmPtrs ptrs, int ab_dtype, int c_dtype, int epilogue, int gemm_variant, int pair_variant, int n_cu) {
  GemmPlan p{};
  p.epilogue = epilogue;
  const int cb = pair_variant == 1 ? 0 : a.c_blocked, ab = pair_variant == 1 ? 0 : a.a_blocked;  // (pair variant 1: the same kernel, row-major)
  const bool f8 = ab_dtype == DFD_FP8;
  if (ab_dtype != DFD_F32) {
    // a q|k|v projection without an export is a plain biased store
    const int epi_p = epilogue == DFD_EPI_QKV_EXPORT && !(ptrs.present & DFD_GEMM_PTR_EXPORT) ? DFD_EPI_BIAS : epilogue;
    int kernel = DFD_GEMM_PINGPONG;
    const char* why = a.pair && f8                ? "the fragment-blocked layout is bf16"
                      : gemm_variant == 1 ? "dfd_gemm_set_variant(1) skips the ping-pong kernel"
                                          : gemm_persistent_refuses(kernel, a, ptrs, f8, c_dtype, epi_p, cb, ab);
    if (why && !a.pair) why = gemm_persistent_refuses(kernel = DFD_GEMM_PERSISTENT, a, ptrs, f8, c_dtype, epi_p, cb, ab);
    if (!why) {
      p.kernel = kernel; p.epilogue = epi_p; p.grid_y = 1; p.block = 512;
      p.c_blocked = cb; p.a_blocked = ab;  // (f32 operands never get here: the general kernel has no layout but row-major)
      // (gemm256p.hip takes spare_cus as given)
      p.tiles = plan_tiles(a.M, a.N, a.spare_cus, kernel == DFD_GEMM_PINGPONG && a.spare_if_free, a.tile_rows, f8, epi_p == DFD_EPI_RESIDUAL_POS, n_cu);
      p.dynamic = kernel == DFD_GEMM_PINGPONG && !f8 && a.K / 64 >= 6 && gemm_variant == 3;
      return p;
    }
    if (a.pair || f8) {  // no other kernel knows the layout / there is no second fp8 kernel
      p.refused = why;
      return p;
    }
    if (!gemm_tile_refuses(a, ptrs, c_dtype, epilogue)) {
      const int tiles_m = (int)((a.M + 255) / 256);
      const int64_t ntiles = (int64_t)tiles_m * (a.N / GEMM_TILE_N);
      p.kernel = DFD_GEMM_TILE; p.tiles = TilePlan{256, tiles_m, ntiles, (int)ntiles}; p.grid_y = 1; p.block = 512;
      return p;
    }
  }
  p.refused = gemm_general_refuses(c_dtype, epilogue);
  if (!p.refused) {
    const int tiles_m = (int)((a.M + 127) / 128), tiles_n = (a.N + 127) / 128;
    p.kernel = DFD_GEMM_GENERAL; p.tiles = TilePlan{128, tiles_m, (int64_t)tiles_m * tiles_n, tiles_n}; p.grid_y = (unsigned)tiles_m; p.block = 256;
  }
  return p;
}

// Launch of one instantiation at the planned grid, and the one report of a failed launch (`kernel`: its name).
template <auto Kernel, typename... A>
int gemm_launch(const char* kernel, const GemmPlan& p, hipStream_t st, const A&... args) {
  hipLaunchKernelGGL(Kernel, dim3((unsigned)p.tiles.grid, p.grid_y), dim3(p.block), 0, st, args...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    dfd_set_error("dfd_gemm(%s): launch failed: %s", kernel, hipGetErrorString(e));
    return DFD_ERR_LAUNCH;
  }
  return DFD_OK;
}

// Each file exports one launcher for the plans of its kernel; none decides.  They map (epilogue, C type, operand type, tile
// height, blocked A) to an instantiation and may complete the argument block (row -> frame dividers, the tile counters).
int dfd_gemm256_launch(const GemmPlan& p, const GemmArgs& a, int c_dtype, hipStream_t st);            // gemm256.hip: DFD_GEMM_TILE
int dfd_gemm256p_launch(const GemmPlan& p, GemmArgs& a, bool f8, bool cf8, hipStream_t st);           // gemm256p.hip: DFD_GEMM_PERSISTENT
int dfd_gemm256e_launch(const GemmPlan& p, GemmArgs& a, bool f8, bool cf8, hipStream_t st);           // gemm256e.hip: DFD_GEMM_PINGPONG
