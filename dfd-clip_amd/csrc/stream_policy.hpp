// The cache policy of the read-once streams (dfd_stream_policy_set of include/dfdclip_hooks.h), in one place.
//
// A kernel that touches each byte once (the decoder's K/V pass and weight streams, the optimizer, the encoder's row
// kernels) takes a `template <bool NT>`; its launcher picks the instantiation from its family's bit of the process-wide
// mask at launch time (a captured graph keeps what was set at capture).  NT = true issues the non-temporal form of the
// load or store (`nt` on the global_load / global_store), NT = false the plain form the kernel had before: the `false`
// instantiation is that kernel, instruction for instruction.  Values are never changed, only the policy bit.
// Vector memory instructions only.
#pragma once
#include "common.hpp"
#include "../../include/dfdclip_hooks.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

// host: is this family's bit set right now?
bool dfd_stream_on(unsigned family_bit);

template <bool NT, typename V> __device__ __forceinline__ V stream_load(const V* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT, typename V> __device__ __forceinline__ void stream_store(V* p, V v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// 16 / 8 / 4 bytes as f32 lanes; a bf16 reader bit-casts (bf16x8 from 16 bytes, bf16x4 from 8)
template <bool NT> __device__ __forceinline__ f32x4 stream_load16(const void* p) { return stream_load<NT>(static_cast<const f32x4*>(p)); }
template <bool NT> __device__ __forceinline__ f32x2 stream_load8(const void* p) { return stream_load<NT>(static_cast<const f32x2*>(p)); }
template <bool NT> __device__ __forceinline__ float stream_load4(const float* p) { return stream_load<NT>(p); }
template <bool NT> __device__ __forceinline__ void stream_store16(void* p, f32x4 v) { stream_store<NT>(static_cast<f32x4*>(p), v); }
template <bool NT> __device__ __forceinline__ void stream_store4(float* p, float v) { stream_store<NT>(p, v); }
