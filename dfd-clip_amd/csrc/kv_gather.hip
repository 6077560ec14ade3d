// dfd_kv_gather_patches (include/dfdclip_kvgather.h): the kept patch rows of K and V of every tapped layer, gathered out of
// the q|k|v activations (or a dense export) into compact [L, frames*S, D] tensors, with the temporal positional embedding
// added on the way when the decoder reads them next.  A pure byte mover: one row is D elements (1,536 B at ViT-B in bf16),
// read once, written once.  As in swiglu.hip a block of 256 lanes covers `tpr` lanes per row (a power of two) and 256 / tpr
// rows, and a lane walks its row in steps of tpr chunks, so a wave's accesses within a row are consecutive 16-byte pieces.
// A lane moves the K piece and the V piece of the same row: one index lookup and one offset serve both, and two loads are
// in flight per lane.  blockIdx.y is the layer, so the row -> (frame, kept position) split is one 32-bit division per lane.
// No LDS, no atomics; the patch position is clamped to [0, P) before any address is formed.
#include "common.hpp"
#include "stream_policy.hpp"
#include "../../include/dfdclip_kvgather.h"

namespace {

constexpr int kBlock = 256;

template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int n = 4; };
template <> struct Vec16<bf16_t> { static constexpr int n = 8; };

// The one arithmetic of both forms: pos is rounded to the tensor type first, then one f32 add and one rounding.
template <typename T> __device__ __forceinline__ T add_pos(T a, float p) { return from_f32<T>(to_f32(a) + to_f32(from_f32<T>(p))); }

// 16 bytes of a row plus the 8 (bf16: p0 | p1) or 4 (f32: p0) entries of pos under them
__device__ __forceinline__ f32x4 add_pos16(f32x4 a, f32x4 p0, f32x4 p1, bf16_t) {
  const bf16x8 av = __builtin_bit_cast(bf16x8, a);
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[i] = add_pos<bf16_t>(av[i], p0[i]);
    o[i + 4] = add_pos<bf16_t>(av[i + 4], p1[i]);
  }
  return __builtin_bit_cast(f32x4, o);
}
__device__ __forceinline__ f32x4 add_pos16(f32x4 a, f32x4 p0, f32x4, float) {
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = add_pos<float>(a[i], p0[i]);
  return o;
}

// What a lane needs to know about its row: the source offset (shared by K and V), the output offset, the pos row.
struct Row {
  int64_t src, dst;
  int t;
};

__device__ __forceinline__ bool locate(Row& row, int tpr_log2, int64_t sl, int64_t sf, int64_t sp, const int32_t* __restrict__ index,
                                       uint32_t rows, int Tn, int P, int S, int D) {
  const int64_t r64 = (int64_t)blockIdx.x * (kBlock >> tpr_log2) + (threadIdx.x >> tpr_log2);
  if (r64 >= (int64_t)rows) return false;
  const uint32_t r = (uint32_t)r64, f = r / (uint32_t)S, j = r - f * (uint32_t)S;
  const int64_t l = blockIdx.y;
  int p = index[l * S + j];
  p = p < 0 ? 0 : (p >= P ? P - 1 : p);  // a bad table never leaves the frame's rows
  row.src = l * sl + (int64_t)f * sf + (int64_t)p * sp;
  row.dst = (l * (int64_t)rows + r) * D;
  row.t = (int)(f % (uint32_t)Tn);
  return true;
}

// 16 bytes of the K row and of the V row per lane and step.  cpr = chunks per row (D / Vec16<T>::n).
template <typename T, bool NT, bool POS>
__global__ __launch_bounds__(kBlock) void kv_gather_vec16_kernel(const T* __restrict__ k, const T* __restrict__ v, int64_t sl, int64_t sf,
                                                                 int64_t sp, const int32_t* __restrict__ index,
                                                                 const float* __restrict__ pos, T* __restrict__ k_out,
                                                                 T* __restrict__ v_out, uint32_t rows, int Tn, int P, int S, int D, int cpr,
                                                                 int tpr_log2) {
  constexpr int V = Vec16<T>::n;
  Row row;
  if (!locate(row, tpr_log2, sl, sf, sp, index, rows, Tn, P, S, D)) return;
  const int tpr = 1 << tpr_log2;
  const T* kr = k + row.src;
  const T* vr = v + row.src;
  T* ko = k_out + row.dst;
  T* vo = v_out + row.dst;
  const float* pr = POS ? pos + (int64_t)row.t * D : nullptr;
#pragma unroll 2
  for (int c = threadIdx.x & (tpr - 1); c < cpr; c += tpr) {
    const int64_t e = (int64_t)c * V;
    f32x4 a = stream_load16<NT>(kr + e);
    f32x4 b = stream_load16<NT>(vr + e);
    if constexpr (POS) {
      const f32x4 p0 = *reinterpret_cast<const f32x4*>(pr + e);
      f32x4 p1 = p0;
      if constexpr (V == 8) p1 = *reinterpret_cast<const f32x4*>(pr + e + 4);
      a = add_pos16(a, p0, p1, T{});
      b = add_pos16(b, p0, p1, T{});
    }
    *reinterpret_cast<f32x4*>(ko + e) = a;
    *reinterpret_cast<f32x4*>(vo + e) = b;
  }
}

// One element of each row per lane and step: any D, any alignment.
template <typename T, bool NT, bool POS>
__global__ __launch_bounds__(kBlock) void kv_gather_element_kernel(const T* __restrict__ k, const T* __restrict__ v, int64_t sl, int64_t sf,
                                                                   int64_t sp, const int32_t* __restrict__ index,
                                                                   const float* __restrict__ pos, T* __restrict__ k_out,
                                                                   T* __restrict__ v_out, uint32_t rows, int Tn, int P, int S, int D,
                                                                   int tpr_log2) {
  Row row;
  if (!locate(row, tpr_log2, sl, sf, sp, index, rows, Tn, P, S, D)) return;
  const int tpr = 1 << tpr_log2;
  const T* kr = k + row.src;
  const T* vr = v + row.src;
  T* ko = k_out + row.dst;
  T* vo = v_out + row.dst;
  const float* pr = POS ? pos + (int64_t)row.t * D : nullptr;
  for (int c = threadIdx.x & (tpr - 1); c < D; c += tpr) {
    T a = stream_load<NT>(kr + c);
    T b = stream_load<NT>(vr + c);
    if constexpr (POS) {
      const float p = pr[c];
      a = add_pos<T>(a, p);
      b = add_pos<T>(b, p);
    }
    ko[c] = a;
    vo[c] = b;
  }
}

// lanes per row: the smallest power of two that covers `items`, at most the block
int lanes_log2(int items) {
  int l = 0;
  while (l < 8 && (1 << l) < items) ++l;
  return l;
}

thread_local int g_last_path = 0;

struct Args {
  const void *k, *v;
  int64_t sl, sf, sp;
  const int32_t* index;
  const float* pos;
  void *k_out, *v_out;
  int L;
  int64_t frames;
  int T, P, S, D;
};

template <typename T, bool NT, bool POS>
void launch_form(const Args& a, bool vec, hipStream_t st) {
  constexpr int V = Vec16<T>::n;
  const uint32_t rows = (uint32_t)(a.frames * a.S);
  const int l2 = lanes_log2(vec ? a.D / V : a.D);
  const uint32_t rpb = kBlock >> l2;
  const dim3 grid((rows + rpb - 1) / rpb, (unsigned)a.L), block(kBlock);
  const T* k = static_cast<const T*>(a.k);
  const T* v = static_cast<const T*>(a.v);
  T* ko = static_cast<T*>(a.k_out);
  T* vo = static_cast<T*>(a.v_out);
  if (vec)
    hipLaunchKernelGGL((kv_gather_vec16_kernel<T, NT, POS>), grid, block, 0, st, k, v, a.sl, a.sf, a.sp, a.index, a.pos, ko, vo, rows, a.T,
                       a.P, a.S, a.D, a.D / V, l2);
  else
    hipLaunchKernelGGL((kv_gather_element_kernel<T, NT, POS>), grid, block, 0, st, k, v, a.sl, a.sf, a.sp, a.index, a.pos, ko, vo, rows, a.T,
                       a.P, a.S, a.D, l2);
}

template <typename T>
int launch(const Args& a, hipStream_t st) {
  constexpr int V = Vec16<T>::n;
  const bool nt = dfd_stream_on(DFD_STREAM_DECODER_KV);
  const bool vec = a.D % V == 0 && a.sl % V == 0 && a.sf % V == 0 && a.sp % V == 0 && dfd_aligned16(a.k) && dfd_aligned16(a.v) &&
                   dfd_aligned16(a.k_out) && dfd_aligned16(a.v_out) && (a.pos == nullptr || dfd_aligned16(a.pos));
  const bool pos = a.pos != nullptr;
  if (nt) {
    if (pos) launch_form<T, true, true>(a, vec, st);
    else launch_form<T, true, false>(a, vec, st);
  } else {
    if (pos) launch_form<T, false, true>(a, vec, st);
    else launch_form<T, false, false>(a, vec, st);
  }
  DFD_CHECK_LAUNCH("dfd_kv_gather_patches");
  g_last_path = vec ? DFD_KVGATHER_VEC16 : DFD_KVGATHER_ELEMENT;
  return DFD_OK;
}

}  // namespace

extern "C" int dfd_kv_gather_patches(const void* k, const void* v, int dtype, int64_t stride_layer, int64_t stride_frame, int64_t stride_patch,
                                     const int32_t* index, const float* pos, void* k_out, void* v_out, int L, int64_t frames, int T, int P,
                                     int S, int D, void* stream) {
  g_last_path = 0;
  DFD_REQUIRE(dtype == DFD_F32 || dtype == DFD_BF16, "dfd_kv_gather_patches: dtype %d unsupported (DFD_F32 or DFD_BF16, for all four tensors)",
              dtype);
  DFD_REQUIRE(k != nullptr && v != nullptr && index != nullptr && k_out != nullptr && v_out != nullptr,
              "dfd_kv_gather_patches: null pointer (k=%p v=%p index=%p k_out=%p v_out=%p)", k, v, (const void*)index, k_out, v_out);
  DFD_REQUIRE(L >= 0 && frames >= 0 && P >= 0 && D >= 0, "dfd_kv_gather_patches: negative size (L=%d frames=%lld P=%d D=%d)", L,
              (long long)frames, P, D);
  DFD_REQUIRE(S >= 0 && S <= P, "dfd_kv_gather_patches: S=%d outside [0, P=%d]: at most every patch row can be kept", S, P);
  DFD_REQUIRE(T > 0 && frames % T == 0, "dfd_kv_gather_patches: frames=%lld is no multiple of T=%d (T > 0: whole clips)", (long long)frames, T);
  DFD_REQUIRE(stride_patch >= D && stride_frame >= 0 && stride_layer >= 0,
              "dfd_kv_gather_patches: strides (layer %lld, frame %lld, patch %lld): stride_patch >= D=%d and none negative",
              (long long)stride_layer, (long long)stride_frame, (long long)stride_patch, D);
  DFD_REQUIRE(L <= 65535 && D < (1 << 30) && frames < (1ll << 31) && frames * (int64_t)(S > 0 ? S : 1) < (1ll << 31),
              "dfd_kv_gather_patches: L=%d, frames*S=%lld*%d, D=%d do not fit the grid (L <= 65535, frames*S < 2^31, D < 2^30)", L,
              (long long)frames, S, D);
  if (L == 0 || frames == 0 || S == 0) return DFD_OK;
  DFD_REQUIRE(D > 0, "dfd_kv_gather_patches: D=%d: a row needs at least one element", D);
  const Args a{k, v, stride_layer, stride_frame, stride_patch, index, pos, k_out, v_out, L, frames, T, P, S, D};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == DFD_BF16 ? launch<bf16_t>(a, st) : launch<float>(a, st);
}

extern "C" int dfd_kv_gather_last_path(void) { return g_last_path; }
