// What adapter.hip and adapter_structs.hip share: the 4- and 8-wide vector access (Vec), the block reduction of the
// statistics kernels (block_sum), the way from two dtype codes to template arguments (with_types) and the two argument
// rules every entry point of the family repeats (ok_dtype, check_drop).
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.hpp"

// N = 4 or 8 consecutive elements of float or bf16 as floats: f32 moves 16 bytes per access (two accesses for N = 8),
// bf16 moves all N elements in one access of 8 or 16 bytes.  p must be aligned to the access.
template <typename T, int N> struct Vec {
  static_assert((N == 4 || N == 8) && (std::is_same_v<T, float> || std::is_same_v<T, bf16_t>), "Vec: float or bf16_t, 4 or 8 wide");
  static constexpr int W = std::is_same_v<T, float> ? 4 : N;  // elements per access
  using Raw = std::conditional_t<std::is_same_v<T, float>, f32x4, std::conditional_t<N == 8, bf16x8, bf16x4>>;
  static __device__ __forceinline__ void load(const T* p, float* o) {
#pragma unroll
    for (int k = 0; k < N; k += W) {
      const Raw r = *reinterpret_cast<const Raw*>(p + k);
#pragma unroll
      for (int e = 0; e < W; ++e) o[k + e] = (float)r[e];
    }
  }
  static __device__ __forceinline__ void store(T* p, const float* o) {
#pragma unroll
    for (int k = 0; k < N; k += W) {
      Raw r;
#pragma unroll
      for (int e = 0; e < W; ++e) r[e] = (T)o[k + e];
      *reinterpret_cast<Raw*>(p + k) = r;
    }
  }
};

// Sum of v over the workgroup, the same bits in every thread: wave butterfly, lane 0 of wave k to sc[k], then every
// thread adds sc[0..NW) from 0.f upward.  NW > 0: the workgroup is exactly NW waves (all NW slots are read); NW == 0:
// blockDim.x / 64 at run time, for the kernels launched with 64 or 1024 threads.  sc: 16 floats of LDS.
template <int NW = 0> __device__ __forceinline__ float block_sum(float v, float* sc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) sc[wave] = v;
  __syncthreads();
  float t = 0.f;
  if constexpr (NW > 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) t += sc[i];
  } else {
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; ++i) t += sc[i];
  }
  return t;
}

// ---- host ------------------------------------------------------------------------------------------------------------
static inline bool ok_dtype(int d) { return d == DFD_F32 || d == DFD_BF16; }

// The dropout descriptor of an entry point `fn`: none, or 0 <= p < 1 with a generator state wherever p > 0.
static inline int check_drop(const char* fn, const dfd_dropout_t* drop) {
  DFD_REQUIRE(!drop || (drop->p >= 0.f && drop->p < 1.f && (drop->p == 0.f || drop->rng_state)), "%s: bad dropout", fn);
  return DFD_OK;
}

// f(Type<A>{}, Type<B>{}) with the element types of two dtype codes, each DFD_F32 or DFD_BF16 (the caller has checked).
// ALL = false leaves (bf16, f32) out, for the entry points whose first operand has the second's type or is f32: no
// kernel is instantiated for a pair they refuse.
template <typename T> struct Type { using type = T; };
template <bool ALL = true, typename F> void with_types(int code_a, int code_b, F&& f) {
  if (code_a == DFD_F32) code_b == DFD_F32 ? f(Type<float>{}, Type<float>{}) : f(Type<float>{}, Type<bf16_t>{});
  else if constexpr (ALL) code_b == DFD_F32 ? f(Type<bf16_t>{}, Type<float>{}) : f(Type<bf16_t>{}, Type<bf16_t>{});
  else f(Type<bf16_t>{}, Type<bf16_t>{});
}
