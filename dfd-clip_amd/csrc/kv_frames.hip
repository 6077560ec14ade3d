// dfd_kv_move_frames (include/dfdclip_kvframes.h): whole frames of K and V of every tapped layer moved between two strided
// layouts, with a frame table on either side.  The streaming path uses it twice: to ingest the raw rows of a tower pass out
// of the in-place q|k|v buffer into the slots of a frame ring, and to gather the frames of W windows out of the ring into a
// dense [L, W*T, P, D] tensor that the decoder reads as it reads any other.  A pure byte mover, shaped as kv_gather.hip: a
// block of 256 lanes covers `tpr` lanes per row (a power of two) and 256 / tpr rows, a lane walks its row in steps of tpr
// chunks, and it moves the K piece and the V piece of the same row, so one pair of table lookups and one pair of offsets
// serve both.  blockIdx.y is the layer, so the row -> (frame, patch) split is one 32-bit division per lane.  No LDS, no
// atomics; both frame numbers are clamped to their range before any address is formed.
#include "common.hpp"
#include "stream_policy.hpp"
#include "../../include/dfdclip_kvframes.h"

namespace {

constexpr int kBlock = 256;

template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int n = 4; };
template <> struct Vec16<bf16_t> { static constexpr int n = 8; };

struct Strides {
  int64_t layer, frame, patch;
};

// What a lane needs to know about its row: the source offset and the destination offset (each shared by K and V).
struct Row {
  int64_t src, dst;
};

__device__ __forceinline__ int clamp_frame(int f, int frames) { return f < 0 ? 0 : (f >= frames ? frames - 1 : f); }

__device__ __forceinline__ bool locate(Row& row, int tpr_log2, Strides s, Strides d, const int32_t* __restrict__ src_frame,
                                       const int32_t* __restrict__ dst_frame, uint32_t rows, int src_frames, int dst_frames, int P) {
  const int64_t r64 = (int64_t)blockIdx.x * (kBlock >> tpr_log2) + (threadIdx.x >> tpr_log2);
  if (r64 >= (int64_t)rows) return false;
  const uint32_t r = (uint32_t)r64, i = r / (uint32_t)P, p = r - i * (uint32_t)P;
  const int64_t l = blockIdx.y;
  // a bad table (or an identity longer than the side it walks) never leaves the tensor's frames
  const int fs = clamp_frame(src_frame ? src_frame[i] : (int)i, src_frames);
  const int fd = clamp_frame(dst_frame ? dst_frame[i] : (int)i, dst_frames);
  row.src = l * s.layer + (int64_t)fs * s.frame + (int64_t)p * s.patch;
  row.dst = l * d.layer + (int64_t)fd * d.frame + (int64_t)p * d.patch;
  return true;
}

// 16 bytes of the K row and of the V row per lane and step.  cpr = chunks per row (D / Vec16<T>::n).
template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) void kv_frames_vec16_kernel(const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ k_out,
                                                                 T* __restrict__ v_out, Strides s, Strides d,
                                                                 const int32_t* __restrict__ src_frame,
                                                                 const int32_t* __restrict__ dst_frame, uint32_t rows, int src_frames,
                                                                 int dst_frames, int P, int cpr, int tpr_log2) {
  constexpr int V = Vec16<T>::n;
  Row row;
  if (!locate(row, tpr_log2, s, d, src_frame, dst_frame, rows, src_frames, dst_frames, P)) return;
  const int tpr = 1 << tpr_log2;
  const T* kr = k + row.src;
  const T* vr = v + row.src;
  T* ko = k_out + row.dst;
  T* vo = v_out + row.dst;
#pragma unroll 2
  for (int c = threadIdx.x & (tpr - 1); c < cpr; c += tpr) {
    const int64_t e = (int64_t)c * V;
    const f32x4 a = stream_load16<NT>(kr + e);
    const f32x4 b = stream_load16<NT>(vr + e);
    *reinterpret_cast<f32x4*>(ko + e) = a;
    *reinterpret_cast<f32x4*>(vo + e) = b;
  }
}

// One element of each row per lane and step: any D, any alignment.
template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) void kv_frames_element_kernel(const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ k_out,
                                                                   T* __restrict__ v_out, Strides s, Strides d,
                                                                   const int32_t* __restrict__ src_frame,
                                                                   const int32_t* __restrict__ dst_frame, uint32_t rows, int src_frames,
                                                                   int dst_frames, int P, int D, int tpr_log2) {
  Row row;
  if (!locate(row, tpr_log2, s, d, src_frame, dst_frame, rows, src_frames, dst_frames, P)) return;
  const int tpr = 1 << tpr_log2;
  const T* kr = k + row.src;
  const T* vr = v + row.src;
  T* ko = k_out + row.dst;
  T* vo = v_out + row.dst;
  for (int c = threadIdx.x & (tpr - 1); c < D; c += tpr) {
    const T a = stream_load<NT>(kr + c);
    const T b = stream_load<NT>(vr + c);
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
  void *k_out, *v_out;
  Strides s, d;
  const int32_t *src_frame, *dst_frame;
  int L;
  int64_t n;
  int src_frames, dst_frames, P, D;
};

template <typename T, bool NT>
void launch_form(const Args& a, bool vec, hipStream_t st) {
  constexpr int V = Vec16<T>::n;
  const uint32_t rows = (uint32_t)(a.n * a.P);
  const int l2 = lanes_log2(vec ? a.D / V : a.D);
  const uint32_t rpb = kBlock >> l2;
  const dim3 grid((rows + rpb - 1) / rpb, (unsigned)a.L), block(kBlock);
  const T* k = static_cast<const T*>(a.k);
  const T* v = static_cast<const T*>(a.v);
  T* ko = static_cast<T*>(a.k_out);
  T* vo = static_cast<T*>(a.v_out);
  if (vec)
    hipLaunchKernelGGL((kv_frames_vec16_kernel<T, NT>), grid, block, 0, st, k, v, ko, vo, a.s, a.d, a.src_frame, a.dst_frame, rows,
                       a.src_frames, a.dst_frames, a.P, a.D / V, l2);
  else
    hipLaunchKernelGGL((kv_frames_element_kernel<T, NT>), grid, block, 0, st, k, v, ko, vo, a.s, a.d, a.src_frame, a.dst_frame, rows,
                       a.src_frames, a.dst_frames, a.P, a.D, l2);
}

bool multiples_of(const Strides& s, int v) { return s.layer % v == 0 && s.frame % v == 0 && s.patch % v == 0; }

template <typename T>
int launch(const Args& a, bool src_once, hipStream_t st) {
  constexpr int V = Vec16<T>::n;
  const bool nt = src_once && dfd_stream_on(DFD_STREAM_DECODER_KV);
  const bool vec = a.D % V == 0 && multiples_of(a.s, V) && multiples_of(a.d, V) && dfd_aligned16(a.k) && dfd_aligned16(a.v) &&
                   dfd_aligned16(a.k_out) && dfd_aligned16(a.v_out);
  if (nt) launch_form<T, true>(a, vec, st);
  else launch_form<T, false>(a, vec, st);
  DFD_CHECK_LAUNCH("dfd_kv_move_frames");
  g_last_path = vec ? DFD_KVFRAMES_VEC16 : DFD_KVFRAMES_ELEMENT;
  return DFD_OK;
}

}  // namespace

extern "C" int dfd_kv_move_frames(const void* k, const void* v, void* k_out, void* v_out, int dtype, int64_t src_stride_layer,
                                  int64_t src_stride_frame, int64_t src_stride_patch, int64_t dst_stride_layer, int64_t dst_stride_frame,
                                  int64_t dst_stride_patch, const int32_t* src_frame, const int32_t* dst_frame, int L, int64_t n,
                                  int src_frames, int dst_frames, int P, int D, int flags, void* stream) {
  g_last_path = 0;
  DFD_REQUIRE(dtype == DFD_F32 || dtype == DFD_BF16, "dfd_kv_move_frames: dtype %d unsupported (DFD_F32 or DFD_BF16, for all four tensors)",
              dtype);
  DFD_REQUIRE(k != nullptr && v != nullptr && k_out != nullptr && v_out != nullptr,
              "dfd_kv_move_frames: null pointer (k=%p v=%p k_out=%p v_out=%p)", k, v, k_out, v_out);
  DFD_REQUIRE((flags & ~DFD_KVFRAMES_SRC_ONCE) == 0, "dfd_kv_move_frames: unknown flag bits in flags=0x%x (DFD_KVFRAMES_SRC_ONCE = 1 is all)",
              (unsigned)flags);
  DFD_REQUIRE(L >= 0 && n >= 0 && P >= 0 && D >= 0 && src_frames >= 0 && dst_frames >= 0,
              "dfd_kv_move_frames: negative size (L=%d n=%lld src_frames=%d dst_frames=%d P=%d D=%d)", L, (long long)n, src_frames,
              dst_frames, P, D);
  DFD_REQUIRE(src_stride_patch >= D && src_stride_frame >= 0 && src_stride_layer >= 0,
              "dfd_kv_move_frames: source strides (layer %lld, frame %lld, patch %lld): src_stride_patch >= D=%d and none negative",
              (long long)src_stride_layer, (long long)src_stride_frame, (long long)src_stride_patch, D);
  DFD_REQUIRE(dst_stride_patch >= D && dst_stride_frame >= 0 && dst_stride_layer >= 0,
              "dfd_kv_move_frames: destination strides (layer %lld, frame %lld, patch %lld): dst_stride_patch >= D=%d and none negative",
              (long long)dst_stride_layer, (long long)dst_stride_frame, (long long)dst_stride_patch, D);
  DFD_REQUIRE(L <= 65535 && D < (1 << 30) && n < (1ll << 31) && n * (int64_t)(P > 0 ? P : 1) < (1ll << 31),
              "dfd_kv_move_frames: L=%d, n*P=%lld*%d, D=%d do not fit the grid (L <= 65535, n*P < 2^31, D < 2^30)", L, (long long)n, P, D);
  if (L == 0 || n == 0 || P == 0) return DFD_OK;
  DFD_REQUIRE(D > 0, "dfd_kv_move_frames: D=%d: a row needs at least one element", D);
  DFD_REQUIRE(src_frames > 0 && dst_frames > 0, "dfd_kv_move_frames: src_frames=%d, dst_frames=%d: both sides need at least one frame",
              src_frames, dst_frames);
  DFD_REQUIRE((src_frame != nullptr || n <= src_frames) && (dst_frame != nullptr || n <= dst_frames),
              "dfd_kv_move_frames: n=%lld frames under an identity table (NULL) exceed that side (src_frames=%d, dst_frames=%d)",
              (long long)n, src_frames, dst_frames);
  const Args a{k,         v, k_out, v_out, {src_stride_layer, src_stride_frame, src_stride_patch}, {dst_stride_layer, dst_stride_frame, dst_stride_patch},
               src_frame, dst_frame, L, n, src_frames, dst_frames, P, D};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == DFD_BF16 ? launch<bf16_t>(a, (flags & DFD_KVFRAMES_SRC_ONCE) != 0, st) : launch<float>(a, (flags & DFD_KVFRAMES_SRC_ONCE) != 0, st);
}

extern "C" int dfd_kv_move_last_path(void) { return g_last_path; }
