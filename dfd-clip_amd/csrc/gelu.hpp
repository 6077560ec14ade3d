// nn.GELU() (the erf form): gelu(x) = x * Phi(x), Phi the standard normal distribution function.  ONE device function
// for every kernel that needs it: the GEMM epilogue DFD_EPI_BIAS_GELU (DINOv2's fc1; gemm.hip, gemm256e.hip) and the
// adapter's GELU kernels (adapter_structs.hip), so they agree bit for bit.
//
// Phi(-|x|) = erfc(|x| / sqrt 2) / 2 by Abramowitz & Stegun 7.1.26: erfc(z) = t (a1 + t (a2 + t (a3 + t (a4 + t a5)))) e^(-z^2),
// t = 1 / (1 + p z), |error| <= 1.5e-7 on erfc.  One v_rcp_f32, one v_exp_f32, and ten plain f32 operations per element,
// no branch; libm's erff costs twice the vector instructions (two polynomial ranges, both executed by a divergent
// wave).  Working from the TAIL keeps the error of gelu small where 1 + erf cancels: measured over [-8, 8] in f32
// against float64, max |error| 4.2e-7 (torch's own f32 GELU: 1.2e-6).
#pragma once

__device__ __forceinline__ float dfd_norm_cdf_tail(float ax) {  // Phi(-ax), ax >= 0
  const float z = ax * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, z, 1.0f));
  const float e = __builtin_amdgcn_exp2f(z * z * -1.4426950408889634f);
  float p = __builtin_fmaf(1.061405429f, t, -1.453152027f);
  p = __builtin_fmaf(p, t, 1.421413741f);
  p = __builtin_fmaf(p, t, -0.284496736f);
  p = __builtin_fmaf(p, t, 0.254829592f);
  return 0.5f * p * t * e;
}
__device__ __forceinline__ float dfd_norm_cdf(float x) {
  const float h = dfd_norm_cdf_tail(__builtin_fabsf(x));
  return x < 0.f ? h : 1.0f - h;
}
__device__ __forceinline__ float gelu_erf(float x) { return x * dfd_norm_cdf(x); }
// The same operations in the same order on a 4-wide accumulator fragment (the compiler pairs them into packed f32
// instructions; every operation is correctly rounded either way, so this returns gelu_erf of each element bit for bit).
typedef float dfd_gelu_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ dfd_gelu_f32x4 gelu_erf4(dfd_gelu_f32x4 x) {
  const dfd_gelu_f32x4 z = __builtin_elementwise_abs(x) * 0.70710678118654752f;
  dfd_gelu_f32x4 t = __builtin_elementwise_fma(dfd_gelu_f32x4(0.3275911f), z, dfd_gelu_f32x4(1.0f));
  dfd_gelu_f32x4 e = z * z * -1.4426950408889634f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    t[i] = __builtin_amdgcn_rcpf(t[i]);
    e[i] = __builtin_amdgcn_exp2f(e[i]);
  }
  dfd_gelu_f32x4 p = __builtin_elementwise_fma(dfd_gelu_f32x4(1.061405429f), t, dfd_gelu_f32x4(-1.453152027f));
  p = __builtin_elementwise_fma(p, t, dfd_gelu_f32x4(1.421413741f));
  p = __builtin_elementwise_fma(p, t, dfd_gelu_f32x4(-0.284496736f));
  p = __builtin_elementwise_fma(p, t, dfd_gelu_f32x4(0.254829592f));
  const dfd_gelu_f32x4 h = 0.5f * p * t * e;
  const dfd_gelu_f32x4 g = 1.0f - h;
  dfd_gelu_f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = x[i] * (x[i] < 0.f ? h[i] : g[i]);
  return r;
}
// d/dz gelu(z) = Phi(z) + z phi(z)
__device__ __forceinline__ float gelu_erf_grad(float z) {
  return dfd_norm_cdf(z) + z * 0.3989422804014327f * __builtin_amdgcn_exp2f(z * z * -0.7213475204444817f);
}
