// The encoder's LayerNorm family (fp32 statistics) — HBM-bound row kernels that sit between two GEMMs.
//
// One 64-lane wave per row; the row lives in registers (float4 per lane per 256-column slab), so it is read once and
// written once.  Two-pass statistics in registers (mean, then centred sum of squares), biased variance, eps inside the
// sqrt: the reference's nn.LayerNorm on fp32 (clip/model.py:157-163).
//   dfd_layernorm      y = LN(x)                             bytes per row: cols * (4 + sizeof(y))
//   dfd_layernorm2     x <- LN_a(x) in place, y = LN_b(x)    cols * (4 + 4 + sizeof(y))
//   dfd_add_layernorm  x += delta [+ delta2], y = LN(x)      cols * (4 + sizeof(delta) [* 2] + 4 + sizeof(y))
// and the _dual twin of each, which writes y as bf16 and as e4m3 from the same registers.
// Written once: the row front (ln_fill_mean, ln_rstd, ln_affine) that the kernels are made of (the plain kernel spells the
// same statements out, see there), the output store (store_row4, LnStore), the argument rules (ln_check) and the way from
// a call to an instantiation (ln_launch).
#include <initializer_list>
#include <type_traits>

#include "stream_policy.hpp"
#include "../../include/dfdclip_ext.h"

// e4m3 output (the A operand of an fp8 GEMM, dfd_gemm_fp8): stored value = e4m3(y * inv_scale), saturated at +-448
struct fp8_t {
  unsigned char v;
};

template <typename OutT>
__device__ __forceinline__ void store_row4(OutT* p, f32x4 o, float inv_scale) {
  if constexpr (sizeof(OutT) == 4) {
    *reinterpret_cast<f32x4*>(p) = o;
  } else if constexpr (sizeof(OutT) == 2) {
    bf16x4 ob;
#pragma unroll
    for (int j = 0; j < 4; ++j) ob[j] = (bf16_t)o[j];
    *reinterpret_cast<bf16x4*>(p) = ob;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __builtin_fminf(__builtin_fmaxf(o[j] * inv_scale, -448.0f), 448.0f);
    unsigned pk = __builtin_amdgcn_cvt_pk_fp8_f32(o[0], o[1], 0u, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(o[2], o[3], pk, true);
    *reinterpret_cast<unsigned*>(p) = pk;
  }
}

// ---- the row front ---------------------------------------------------------------------------
// Lane `lane` of the row's wave owns columns c = (i * 64 + lane) * 4 .. c + 3 of slab i, in v[i]; slabs past `cols` hold
// zeros.  Every floating-point expression below is one statement in one operand order, so contraction into FMAs cannot
// differ between callers: the tests ask that layernorm2 equals two layernorm calls, a dual form its single twin and the NT
// form the plain one, bit for bit.
//
// fill(i, c) leaves slab i of the row in v[i].  Returns the row's mean.
template <int SLABS, typename Fill>
__device__ __forceinline__ float ln_fill_mean(f32x4 (&v)[SLABS], int lane, int cols, Fill fill) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < SLABS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < cols) {
      fill(i, c);
      s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    } else {
      v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  return wave_sum(s) / (float)cols;
}

template <int SLABS>
__device__ __forceinline__ float ln_rstd(const f32x4 (&v)[SLABS], int lane, int cols, float mean, float eps) {
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < SLABS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < cols) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = v[i][j] - mean;
        q += d * d;
      }
    }
  }
  return rsqrtf(wave_sum(q) / (float)cols + eps);
}

// emit(i, c, o) takes the four normalised values of slab i; it may write v[i]
template <int SLABS, typename Emit>
__device__ __forceinline__ void ln_affine(f32x4 (&v)[SLABS], int lane, int cols, float mean, float rstd,
                                          const float* __restrict__ gamma, const float* __restrict__ beta, Emit emit) {
#pragma unroll
  for (int i = 0; i < SLABS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < cols) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
      const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (v[i][j] - mean) * rstd * g[j] + b[j];
      emit(i, c, o);
    }
  }
}

// The emit of a row's last LayerNorm: y, which the next GEMM reads, always takes the plain store.
// DUAL: the row is also written as e4m3 to y8 (row stride ldy8) from the registers that hold the normalised f32 values —
// OutT is bf16 then, and inv_scale belongs to y8.  A "kv-bf16" layer of the fp8 encoder reads its LayerNorm output in both
// formats (encoder.py); a second LayerNorm call would read the f32 residual stream once more.
template <typename OutT, bool DUAL>
struct LnStore {
  OutT* yr;
  fp8_t* y8r;
  float inv_scale;
  __device__ __forceinline__ LnStore(OutT* y, int64_t ldy, fp8_t* y8, int64_t ldy8, int64_t row, float inv_scale)
      : yr(y + row * ldy), y8r(DUAL ? y8 + row * ldy8 : nullptr), inv_scale(inv_scale) {}
  __device__ __forceinline__ void operator()(int, int c, f32x4 o) const {
    store_row4(yr + c, o, inv_scale);
    if constexpr (DUAL) store_row4(y8r + c, o, inv_scale);
  }
};

// ---- the three kernels -----------------------------------------------------------------------
// NT (DFD_STREAM_ENCODER_ROWS): the f32 residual stream x and the pending deltas are read once and x is written once, with
// non-temporal loads and stores.
//
// The plain kernel keeps the front spelled out, statement for statement what ln_fill_mean (with a plain load), ln_rstd and
// ln_affine (with LnStore) hold: built from the helpers the compiler schedules it differently, and its 3-slab form (768
// columns, 94,560 rows) measured 0.2 to 0.3 us in 75 slower than this body in two jobs out of two; the evidence
// (profiles/layernorm_front_refactor.txt) also says why that is worth a second try.  test_layernorm2_is_two_layernorms
// holds the two copies to the same bits.
template <typename OutT, int SLABS, bool DUAL = false, bool NT = false>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* __restrict__ x, int64_t ldx,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, OutT* __restrict__ y,
                                                             int64_t ldy, int64_t rows, int cols, float eps, float inv_scale,
                                                             fp8_t* __restrict__ y8 = nullptr, int64_t ldy8 = 0) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * ldx;
  f32x4 v[SLABS];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < SLABS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < cols) {
      v[i] = stream_load16<NT>(xr + c);
      s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    } else {
      v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  const float mean = wave_sum(s) / (float)cols;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < SLABS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < cols) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = v[i][j] - mean;
        q += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)cols + eps);
  OutT* yr = y + row * ldy;
#pragma unroll
  for (int i = 0; i < SLABS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < cols) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
      const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (v[i][j] - mean) * rstd * g[j] + b[j];
      store_row4(yr + c, o, inv_scale);
      if constexpr (DUAL) store_row4(y8 + row * ldy8 + c, o, inv_scale);
    }
  }
}

// Two LayerNorms back to back over the same rows in one pass: x <- LN_a(x) (f32, in place), y = LN_b(x).  The
// encoder's ln_pre followed by the first block's ln_1 (clip/model.py:292, :221): the row stays in registers between
// the two, so x is read once instead of twice.
template <typename OutT, int SLABS, bool DUAL = false, bool NT = false>
__global__ __launch_bounds__(256) void layernorm2_rows_kernel(float* __restrict__ x, int64_t ldx, const float* __restrict__ ga,
                                                              const float* __restrict__ ba, const float* __restrict__ gb,
                                                              const float* __restrict__ bb, OutT* __restrict__ y, int64_t ldy,
                                                              int64_t rows, int cols, float eps, float inv_scale,
                                                              fp8_t* __restrict__ y8 = nullptr, int64_t ldy8 = 0) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* xr = x + row * ldx;
  f32x4 v[SLABS];
  const LnStore<OutT, DUAL> store(y, ldy, y8, ldy8, row, inv_scale);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const float mean = ln_fill_mean<SLABS>(v, lane, cols, [&](int i, int c) {
      if (pass == 0) v[i] = stream_load16<NT>(xr + c);
    });
    const float rstd = ln_rstd<SLABS>(v, lane, cols, mean, eps);
    ln_affine<SLABS>(v, lane, cols, mean, rstd, pass == 0 ? ga : gb, pass == 0 ? ba : bb, [&](int i, int c, f32x4 o) {
      if (pass == 0) {
        stream_store16<NT>(xr + c, o);
        v[i] = o;
      } else {
        store(i, c, o);
      }
    });
  }
}

// Residual add + LayerNorm: x[row] += delta[row] (+ delta2[row]) on the f32 residual stream, stored back when store_x,
// y[row] = LayerNorm(x[row]).  The bf16 encoder path lets out_proj / c_proj write their output as a bf16 `delta` with a
// plain store epilogue instead of a read-modify-write of the f32 stream inside the GEMM (a 128 MB burst per wave of tiles
// with every CU in its epilogue at once), and folds the add into the LayerNorm that follows — exactly torch autocast's
// dataflow (Linear output in bf16, added to the fp32 stream).
template <typename DeltaT, typename OutT, int SLABS, bool DUAL = false, bool NT = false>
__global__ __launch_bounds__(256) void add_layernorm_rows_kernel(float* __restrict__ x, int64_t ldx,
                                                                 const DeltaT* __restrict__ delta, int64_t ldd,
                                                                 const DeltaT* __restrict__ delta2, int store_x,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, OutT* __restrict__ y,
                                                                 int64_t ldy, int64_t rows, int cols, float eps, float inv_scale,
                                                                 fp8_t* __restrict__ y8 = nullptr, int64_t ldy8 = 0) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* xr = x + row * ldx;
  const DeltaT* dr = delta + row * ldd;
  f32x4 v[SLABS];
  const float mean = ln_fill_mean<SLABS>(v, lane, cols, [&](int i, int c) {
    v[i] = stream_load16<NT>(xr + c);
    auto add = [&](const DeltaT* p) {
      if constexpr (sizeof(DeltaT) == 4) {
        const f32x4 d = stream_load16<NT>(p + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] += d[j];
      } else {
        const bf16x4 d = __builtin_bit_cast(bf16x4, stream_load8<NT>(p + c));
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] += (float)d[j];
      }
    };
    add(dr);                                         // (x + delta) + delta2: the order of the two
    if (delta2 != nullptr) add(delta2 + row * ldd);  // separate adds it replaces
    if (store_x) stream_store16<NT>(xr + c, v[i]);
  });
  const float rstd = ln_rstd<SLABS>(v, lane, cols, mean, eps);
  ln_affine<SLABS>(v, lane, cols, mean, rstd, gamma, beta, LnStore<OutT, DUAL>(y, ldy, y8, ldy8, row, inv_scale));
}

// ---- host: one call description, one check, one launch ------------------------------------------
enum LnKind { LN_PLAIN, LN_TWO, LN_ADD };

struct LnCall {
  const char* who;  // the entry point's name
  LnKind kind;
  bool dual;  // y is y16 (y_dtype = DFD_BF16), and y8 / ldy8 are read
  float* x = nullptr;
  int64_t ldx = 0;
  const float *gamma = nullptr, *beta = nullptr;      // the LayerNorm that feeds y
  const float *gamma_a = nullptr, *beta_a = nullptr;  // LN_TWO: the LayerNorm written back to x
  const void *delta = nullptr, *delta2 = nullptr;     // LN_ADD; delta2 may be NULL
  int64_t ldd = 0;
  int delta_dtype = DFD_F32, store_x = 0;
  void* y = nullptr;
  int64_t ldy = 0;
  int y_dtype = DFD_BF16;
  void* y8 = nullptr;
  int64_t ldy8 = 0;
  int64_t rows = 0;
  int cols = 0;
  float eps = 0.f, inv_scale = 0.f;  // inv_scale: of the e4m3 output, y or y8
};

// Every rule of the six entry points, in one order; rows == 0 is accepted by the caller only after all of them.
//  - cols: a positive multiple of 4, up to 4096 for the plain kind (dfd_layernorm, dfd_layernorm_dual: 16 slabs), up to
//    2048 for the other four (8 slabs).  rows: one workgroup per 4 rows has to fit a grid.
//  - leading dimensions: multiples of 4, at least cols.
//  - alignment: x, gamma and beta 16 bytes (float4 loads); y 8 bytes whether it is bf16 or f32, 4 when it is e4m3, and
//    y8 4; the deltas 8 bytes, whatever their type.
//  - an e4m3 output needs inv_scale > 0.
//  - aliasing: dfd_layernorm alone accepts y == x (f32 in place, as encoder.py and the tests use it: a lane has read its
//    columns before it writes them).  The other five refuse an output that is x or a delta, and the dual forms y16 == y8.
static int ln_check(const LnCall& c) {
  const char* who = c.who;
  const bool fp8 = c.y_dtype == DFD_FP8;
  const int max_cols = c.kind == LN_PLAIN ? 4096 : 2048;
  DFD_REQUIRE(c.x && c.gamma && c.beta && c.y && (!c.dual || c.y8) && (c.kind != LN_TWO || (c.gamma_a && c.beta_a)) &&
                  (c.kind != LN_ADD || c.delta),
              "%s: null pointer", who);
  DFD_REQUIRE(c.rows >= 0 && c.cols > 0 && c.cols % 4 == 0 && c.cols <= max_cols,
              "%s: rows=%lld cols=%d: cols must be a positive multiple of 4, <= %d", who, (long long)c.rows, c.cols, max_cols);
  DFD_REQUIRE(c.rows <= 4 * (int64_t)0x7fffffff, "%s: rows=%lld: one workgroup per 4 rows does not fit a grid of 2^31 - 1", who,
              (long long)c.rows);
  const auto ld_ok = [&](int64_t ld) { return ld >= c.cols && ld % 4 == 0; };
  DFD_REQUIRE(ld_ok(c.ldx) && ld_ok(c.ldy) && (!c.dual || ld_ok(c.ldy8)) && (c.kind != LN_ADD || ld_ok(c.ldd)),
              "%s: bad leading dimension (ldx=%lld ldy=%lld ldy8=%lld ldd=%lld): each must be a multiple of 4, >= cols=%d", who,
              (long long)c.ldx, (long long)c.ldy, (long long)c.ldy8, (long long)c.ldd, c.cols);
  DFD_REQUIRE(c.y_dtype == DFD_F32 || c.y_dtype == DFD_BF16 || fp8, "%s: y_dtype=%d must be f32, bf16 or e4m3", who, c.y_dtype);
  DFD_REQUIRE(c.kind != LN_ADD || c.delta_dtype == DFD_F32 || c.delta_dtype == DFD_BF16, "%s: delta_dtype=%d must be f32 or bf16", who,
              c.delta_dtype);
  DFD_REQUIRE(!(fp8 || c.dual) || c.inv_scale > 0.f, "%s: y_dtype: an e4m3 output needs %s > 0", who, c.dual ? "y8_inv_scale" : "y_inv_scale");
  const auto aligned = [](const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; };
  DFD_REQUIRE(aligned(c.x, 16) && aligned(c.gamma, 16) && aligned(c.beta, 16) && aligned(c.gamma_a, 16) && aligned(c.beta_a, 16),
              "%s: x, gamma and beta must be 16-byte aligned", who);
  DFD_REQUIRE(aligned(c.y, fp8 ? 4 : 8) && aligned(c.y8, 4), "%s: y must be 8-byte aligned (an e4m3 y or y8: 4-byte)", who);
  DFD_REQUIRE(aligned(c.delta, 8) && aligned(c.delta2, 8), "%s: delta and delta2 must be 8-byte aligned", who);
  if (c.kind == LN_PLAIN && !c.dual) return DFD_OK;
  for (const void* out : {static_cast<const void*>(c.y), static_cast<const void*>(c.y8)})
    DFD_REQUIRE(!out || (out != c.x && out != c.delta && out != c.delta2), "%s: an output must not alias x or a delta", who);
  DFD_REQUIRE(c.y != c.y8, "%s: y16 and y8 must not alias", who);
  return DFD_OK;
}

// run-time values to template arguments: f(std::integral_constant<int, slabs>{}) for 1 <= slabs <= MAX, f(tag) for a flag
template <typename T> struct LnType { using type = T; };
template <int MAX, typename F> void ln_slabs(int slabs, F&& f) {
  if constexpr (MAX > 0) slabs == MAX ? f(std::integral_constant<int, MAX>{}) : ln_slabs<MAX - 1>(slabs, f);
}
template <typename F> void ln_flag(bool on, F&& f) { on ? f(std::true_type{}) : f(std::false_type{}); }

// (kind, delta type, out type, dual, slabs, NT bit) -> an instantiation of one of the three kernels, launched under the
// call's name
static int ln_launch(const LnCall& c, hipStream_t st) {
  const dim3 grid((unsigned)((c.rows + 3) / 4)), block(256);
  const int slabs = (c.cols + 255) / 256;
  const float inv_scale = c.dual || c.y_dtype == DFD_FP8 ? c.inv_scale : 1.f;
  fp8_t* y8 = static_cast<fp8_t*>(c.y8);
  const auto with_out = [&](auto&& f) {  // f(out type, DUAL)
    if (c.dual) f(LnType<bf16_t>{}, std::true_type{});
    else if (c.y_dtype == DFD_F32) f(LnType<float>{}, std::false_type{});
    else if (c.y_dtype == DFD_FP8) f(LnType<fp8_t>{}, std::false_type{});
    else f(LnType<bf16_t>{}, std::false_type{});
  };
  with_out([&](auto out, auto dual) {
    using OutT = typename decltype(out)::type;
    constexpr bool DUAL = decltype(dual)::value;
    OutT* y = static_cast<OutT*>(c.y);
    ln_flag(dfd_stream_on(DFD_STREAM_ENCODER_ROWS), [&](auto nt) {
      constexpr bool NT = decltype(nt)::value;
      if (c.kind == LN_PLAIN) {
        ln_slabs<16>(slabs, [&](auto s) {
          hipLaunchKernelGGL((layernorm_rows_kernel<OutT, decltype(s)::value, DUAL, NT>), grid, block, 0, st, c.x, c.ldx, c.gamma, c.beta,
                             y, c.ldy, c.rows, c.cols, c.eps, inv_scale, y8, c.ldy8);
        });
      } else if (c.kind == LN_TWO) {
        ln_slabs<8>(slabs, [&](auto s) {
          hipLaunchKernelGGL((layernorm2_rows_kernel<OutT, decltype(s)::value, DUAL, NT>), grid, block, 0, st, c.x, c.ldx, c.gamma_a,
                             c.beta_a, c.gamma, c.beta, y, c.ldy, c.rows, c.cols, c.eps, inv_scale, y8, c.ldy8);
        });
      } else {
        ln_flag(c.delta_dtype == DFD_F32, [&](auto f32) {
          using DeltaT = std::conditional_t<decltype(f32)::value, float, bf16_t>;
          ln_slabs<8>(slabs, [&](auto s) {
            hipLaunchKernelGGL((add_layernorm_rows_kernel<DeltaT, OutT, decltype(s)::value, DUAL, NT>), grid, block, 0, st, c.x, c.ldx,
                               static_cast<const DeltaT*>(c.delta), c.ldd, static_cast<const DeltaT*>(c.delta2), c.store_x, c.gamma,
                               c.beta, y, c.ldy, c.rows, c.cols, c.eps, inv_scale, y8, c.ldy8);
          });
        });
      }
    });
  });
  DFD_CHECK_LAUNCH(c.who);
  return DFD_OK;
}

static int ln_run(const LnCall& c, void* stream) {
  if (int rc = ln_check(c)) return rc;
  if (c.rows == 0) return DFD_OK;
  return ln_launch(c, static_cast<hipStream_t>(stream));
}

// what all six entry points pass: the rows, the LayerNorm that feeds y, the first output, the extent
static LnCall ln_call(const char* who, LnKind kind, bool dual, const float* x, int64_t ldx, const float* gamma, const float* beta,
                      void* y, int64_t ldy, int y_dtype, int64_t rows, int cols, float eps, float inv_scale) {
  LnCall c{who, kind, dual};
  c.x = const_cast<float*>(x), c.ldx = ldx, c.gamma = gamma, c.beta = beta;
  c.y = y, c.ldy = ldy, c.y_dtype = y_dtype;
  c.rows = rows, c.cols = cols, c.eps = eps, c.inv_scale = inv_scale;
  return c;
}

extern "C" int dfd_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy,
                             int y_dtype, int64_t rows, int cols, float eps, float y_inv_scale, void* stream) {
  return ln_run(ln_call("dfd_layernorm", LN_PLAIN, false, x, ldx, gamma, beta, y, ldy, y_dtype, rows, cols, eps, y_inv_scale), stream);
}

extern "C" int dfd_layernorm2(float* x, int64_t ldx, const float* gamma_a, const float* beta_a, const float* gamma_b,
                              const float* beta_b, void* y, int64_t ldy, int y_dtype, int64_t rows, int cols, float eps,
                              float y_inv_scale, void* stream) {
  LnCall c = ln_call("dfd_layernorm2", LN_TWO, false, x, ldx, gamma_b, beta_b, y, ldy, y_dtype, rows, cols, eps, y_inv_scale);
  c.gamma_a = gamma_a, c.beta_a = beta_a;
  return ln_run(c, stream);
}

extern "C" int dfd_add_layernorm(float* x, int64_t ldx, const void* delta, const void* delta2, int64_t ldd, int delta_dtype,
                                 int store_x, const float* gamma, const float* beta, void* y, int64_t ldy, int y_dtype,
                                 int64_t rows, int cols, float eps, float y_inv_scale, void* stream) {
  LnCall c = ln_call("dfd_add_layernorm", LN_ADD, false, x, ldx, gamma, beta, y, ldy, y_dtype, rows, cols, eps, y_inv_scale);
  c.delta = delta, c.delta2 = delta2, c.ldd = ldd, c.delta_dtype = delta_dtype, c.store_x = store_x;
  return ln_run(c, stream);
}

// ---- dual-output forms: y16 (bf16) and y8 (e4m3 of the same f32 value * y8_inv_scale) in one pass ---------------
// Each output is bit-identical to what the single-output entry point writes for that type; the restrictions are those
// of the single-output twin.
extern "C" int dfd_layernorm_dual(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y16, int64_t ldy16,
                                  void* y8, int64_t ldy8, int64_t rows, int cols, float eps, float y8_inv_scale, void* stream) {
  LnCall c = ln_call("dfd_layernorm_dual", LN_PLAIN, true, x, ldx, gamma, beta, y16, ldy16, DFD_BF16, rows, cols, eps, y8_inv_scale);
  c.y8 = y8, c.ldy8 = ldy8;
  return ln_run(c, stream);
}

extern "C" int dfd_layernorm2_dual(float* x, int64_t ldx, const float* gamma_a, const float* beta_a, const float* gamma_b,
                                   const float* beta_b, void* y16, int64_t ldy16, void* y8, int64_t ldy8, int64_t rows, int cols,
                                   float eps, float y8_inv_scale, void* stream) {
  LnCall c = ln_call("dfd_layernorm2_dual", LN_TWO, true, x, ldx, gamma_b, beta_b, y16, ldy16, DFD_BF16, rows, cols, eps, y8_inv_scale);
  c.gamma_a = gamma_a, c.beta_a = beta_a, c.y8 = y8, c.ldy8 = ldy8;
  return ln_run(c, stream);
}

extern "C" int dfd_add_layernorm_dual(float* x, int64_t ldx, const void* delta, const void* delta2, int64_t ldd, int delta_dtype,
                                      int store_x, const float* gamma, const float* beta, void* y16, int64_t ldy16, void* y8,
                                      int64_t ldy8, int64_t rows, int cols, float eps, float y8_inv_scale, void* stream) {
  LnCall c = ln_call("dfd_add_layernorm_dual", LN_ADD, true, x, ldx, gamma, beta, y16, ldy16, DFD_BF16, rows, cols, eps, y8_inv_scale);
  c.delta = delta, c.delta2 = delta2, c.ldd = ldd, c.delta_dtype = delta_dtype, c.store_x = store_x, c.y8 = y8, c.ldy8 = ldy8;
  return ln_run(c, stream);
}
