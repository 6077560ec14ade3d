// Argument block shared by the GEMM kernels: gemm.hip (general shapes, 128-wide tiles), gemm256.hip (tuned bf16, one
// workgroup per tile) and the two persistent kernels gemm256e.hip / gemm256p.hip (bf16 and e4m3 operands; their shared
// epilogue is in gemm256p_common.hpp).  Which kernel serves a call, and with which tiles: gemm_plan.hpp.
#pragma once
#include "dropout.hpp"

struct GemmArgs {
  const void* A;
  const void* W;
  void* C;
  const float* bias;
  const float* pos;
  const float* cls;
  void* k_export;
  void* v_export;
  const void* residual;  // RESIDUAL_POS: source of the residual (NULL = C itself, in place)
  int64_t lda, ldw, ldc, M;
  int N, K, tokens, frames_per_clip;
  int qkv_first;  // QKV_EXPORT: first column block present (0 = q, 1 = k)
  int stream_out; // DFD_GEMM_STREAM_OUT: non-temporal output stores
  int spare_cus;  // persistent kernel: compute units left free for other streams
  int spare_if_free;  // DFD_GEMM_SPARE_IF_FREE: ... only where that costs no extra round of tiles
  int tile_rows;  // persistent kernel: 0 = choose, 224 / 256 = force that tile height (lab, tests)
  DfdDrop drop;   // RESIDUAL_POS: dropout on the accumulator (element index row*N + col); thr16 == 0: none
  FastDiv div_tokens, div_frames;  // persistent kernels, QKV_EXPORT / RESIDUAL_POS: row -> (frame, token), frame -> frame % T
  const float* col_scale;          // fp8 operands: per output column, activation scale x weight-row scale
  float out_inv_scale;             // fp8 output: stored value = e4m3(result * out_inv_scale)
  // gemm256e.hip, dynamic tile hand-out (set by its launcher): eight monotonic counters, one 128-byte line per XCD label
  // (blockIdx & 7), and the value each held when this launch was enqueued; NULL = tiles are dealt statically
  uint32_t* sched;
  uint32_t sched_base[8];
  int no_dynamic;  // (not read any more: GemmPlan::dynamic decides; kept so that the kernels' argument layout stays as it was)
  // gemm256e.hip, the c_fc -> c_proj pair (gemm_blocked.hpp): C is written / A is read in the fragment-blocked layout.
  // pair: the call is one half of such a pair (DFD_GEMM_C_BLOCKED / DFD_GEMM_A_BLOCKED) — gemm256e.hip serves it, at any
  // M, or it is an error; dfd_gemm_pair_set_variant(1) keeps `pair` and clears the other two (the row-major pair).
  int c_blocked, a_blocked, pair;
};
