// dfd_swiglu_fwd (include/dfdclip_swiglu.h): hidden = silu(x12[:, :H]) * x12[:, H:], the gate between the two Linears of a
// SwiGLU feed-forward (DINOv2 ViT-g/14).  Memory-bound: 3 elements moved per gate and about ten vector instructions, so the
// whole design is the access pattern.  A block of 256 lanes covers `tpr` lanes per row (a power of two, at most 256) and
// 256 / tpr rows; a lane walks its row in steps of tpr chunks, so a wave's loads of either half are consecutive 16-byte
// pieces of one row (or of a few short rows) and no index needs a division.  No LDS, no atomics, nothing between the rows
// is touched.
#include "common.hpp"
#include "stream_policy.hpp"
#include "../../include/dfdclip_swiglu.h"

namespace {

constexpr int kBlock = 256;

// The one arithmetic of both forms: exp through exp2 (relative error ~ |a| * 2^-24), the quotient through v_rcp_f32.
// a -> -inf: exp2 = +inf, rcp = 0, a * 0 = -0.  a -> +inf: exp2 = 0, rcp(1) = 1.  (1 + e) >= 1, so rcp never sees 0.
__device__ __forceinline__ float swiglu_gate(float a, float b) {
  const float e = __builtin_amdgcn_exp2f(a * -1.44269504f);
  return (a * __builtin_amdgcn_rcpf(1.0f + e)) * b;
}

template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int n = 4; };
template <> struct Vec16<bf16_t> { static constexpr int n = 8; };

__device__ __forceinline__ f32x4 gate16(f32x4 a, f32x4 b, float) {
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = swiglu_gate(a[i], b[i]);
  return o;
}
__device__ __forceinline__ f32x4 gate16(f32x4 a, f32x4 b, bf16_t) {
  const bf16x8 av = __builtin_bit_cast(bf16x8, a), bv = __builtin_bit_cast(bf16x8, b);
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = from_f32<bf16_t>(swiglu_gate((float)av[i], (float)bv[i]));
  return __builtin_bit_cast(f32x4, o);
}

// 16 bytes of each half per lane and step.  cpr = chunks per row (H / Vec16<T>::n); tpr_log2: lanes per row.
template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) void swiglu_vec16_kernel(const T* __restrict__ x12, int64_t ldx, T* __restrict__ hidden, int64_t ldh,
                                                              int64_t rows, int H, int cpr, int tpr_log2) {
  constexpr int V = Vec16<T>::n;
  const int tpr = 1 << tpr_log2;
  const int64_t r = (int64_t)blockIdx.x * (kBlock >> tpr_log2) + (threadIdx.x >> tpr_log2);
  if (r >= rows) return;
  const T* xr = x12 + r * ldx;
  T* hr = hidden + r * ldh;
#pragma unroll 2
  for (int c = threadIdx.x & (tpr - 1); c < cpr; c += tpr) {
    const f32x4 a = stream_load16<NT>(xr + (int64_t)c * V);
    const f32x4 b = stream_load16<NT>(xr + H + (int64_t)c * V);
    *reinterpret_cast<f32x4*>(hr + (int64_t)c * V) = gate16(a, b, T{});
  }
}

// One element of each half per lane and step: any H, any alignment.
template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) void swiglu_element_kernel(const T* __restrict__ x12, int64_t ldx, T* __restrict__ hidden, int64_t ldh,
                                                                int64_t rows, int H, int tpr_log2) {
  const int tpr = 1 << tpr_log2;
  const int64_t r = (int64_t)blockIdx.x * (kBlock >> tpr_log2) + (threadIdx.x >> tpr_log2);
  if (r >= rows) return;
  const T* xr = x12 + r * ldx;
  T* hr = hidden + r * ldh;
  for (int c = threadIdx.x & (tpr - 1); c < H; c += tpr)
    hr[c] = from_f32<T>(swiglu_gate(to_f32(stream_load<NT>(xr + c)), to_f32(stream_load<NT>(xr + H + c))));
}

// lanes per row: the smallest power of two that covers `items`, at most the block
int lanes_log2(int items) {
  int l = 0;
  while (l < 8 && (1 << l) < items) ++l;
  return l;
}

thread_local int g_last_path = 0;

template <typename T>
int launch(const void* x12v, int64_t ldx, void* hiddenv, int64_t ldh, int64_t rows, int H, hipStream_t st) {
  constexpr int V = Vec16<T>::n;
  const T* x12 = static_cast<const T*>(x12v);
  T* hidden = static_cast<T*>(hiddenv);
  const bool nt = dfd_stream_on(DFD_STREAM_ENCODER_ROWS);
  const bool vec = H % V == 0 && ldx % V == 0 && ldh % V == 0 && dfd_aligned16(x12v) && dfd_aligned16(hiddenv);
  const int l2 = lanes_log2(vec ? H / V : H);
  const int64_t rpb = kBlock >> l2;
  const dim3 grid((unsigned)((rows + rpb - 1) / rpb)), block(kBlock);
  if (vec) {
    auto kern = nt ? swiglu_vec16_kernel<T, true> : swiglu_vec16_kernel<T, false>;
    hipLaunchKernelGGL(kern, grid, block, 0, st, x12, ldx, hidden, ldh, rows, H, H / V, l2);
  } else {
    auto kern = nt ? swiglu_element_kernel<T, true> : swiglu_element_kernel<T, false>;
    hipLaunchKernelGGL(kern, grid, block, 0, st, x12, ldx, hidden, ldh, rows, H, l2);
  }
  DFD_CHECK_LAUNCH("dfd_swiglu_fwd");
  g_last_path = vec ? DFD_SWIGLU_VEC16 : DFD_SWIGLU_ELEMENT;
  return DFD_OK;
}

}  // namespace

extern "C" int dfd_swiglu_fwd(const void* x12, int64_t ldx, void* hidden, int64_t ldh, int dtype, int64_t rows, int H, void* stream) {
  DFD_REQUIRE(dtype == DFD_F32 || dtype == DFD_BF16, "dfd_swiglu_fwd: dtype %d unsupported (DFD_F32 or DFD_BF16, for both tensors)", dtype);
  DFD_REQUIRE(rows >= 0 && rows < (1ll << 31) && H >= 0 && H < (1 << 30), "dfd_swiglu_fwd: rows=%lld, H=%d out of range (0 <= rows < 2^31, 0 <= H < 2^30)",
              (long long)rows, H);
  DFD_REQUIRE(ldx >= 2 * (int64_t)H, "dfd_swiglu_fwd: ldx=%lld < 2H=%lld: a row of x12 holds both halves", (long long)ldx, 2ll * H);
  DFD_REQUIRE(ldh >= H, "dfd_swiglu_fwd: ldh=%lld < H=%d", (long long)ldh, H);
  DFD_REQUIRE(x12 != nullptr && hidden != nullptr, "dfd_swiglu_fwd: null pointer (x12=%p hidden=%p)", x12, hidden);
  g_last_path = 0;
  if (rows == 0 || H == 0) return DFD_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == DFD_BF16 ? launch<bf16_t>(x12, ldx, hidden, ldh, rows, H, st) : launch<float>(x12, ldx, hidden, ldh, rows, H, st);
}

extern "C" int dfd_swiglu_last_path(void) { return g_last_path; }
