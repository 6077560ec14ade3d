// Encoder self-attention, out = softmax(q kᵀ / √d) v per (frame, head), head_dim = 64
// (reference clip/model.py:188-195).  The [N, tokens, tokens, heads] affinity tensor the
// reference materialises (894 MB per layer at B·T = 480) never exists here.
//
// attn_rows_kernel: general kernel for both dtypes (the f32 parity path and the fallback for
//   shapes the MFMA kernel does not take).  One workgroup per (frame, head); K and V of that
//   head staged once in LDS in their storage dtype; one query row per thread held in
//   registers; keys streamed from LDS as wave-wide broadcasts; online softmax in fp32.
// attn_rows_chunked_kernel: the same arithmetic in the same order per query (attn_row_key), with K and V staged in
//   key chunks inside the key loop, for token counts whose whole K and V do not fit the 160 KiB of LDS (f32 above 320
//   tokens, bf16 above 640).  Bit-identical to the whole-head form wherever both can run.
// The bf16 MFMA kernels live in attention_mfma.hip, attention_mfma_xrow.hip and attention_mfma_any.hip; which kernel serves
// a call is decided in one place, attn_plan (attention_common.hpp; the table is in include/dfdclip_hooks.h).
// dfd_attention_fwd here validates, plans, hands the call to the planned kernel's file and records the path.
#include "attention_common.hpp"

namespace {

template <typename T> struct Vec16;  // 16-byte vector of T
template <> struct Vec16<float> { using type = f32x4; static constexpr int N = 4; };
template <> struct Vec16<bf16_t> { using type = bf16x8; static constexpr int N = 8; };

// One key of the online softmax of one query row: q is pre-scaled, Kp / Vp point at the key's 64 channels in LDS.
template <typename T>
__device__ __forceinline__ void attn_row_key(const float (&q)[HD], float (&acc)[HD], float& mx, float& l, const T* Kp, const T* Vp) {
  using V16 = typename Vec16<T>::type;
  constexpr int VN = Vec16<T>::N;
  constexpr int CHUNKS = HD / VN;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int ch = 0; ch < CHUNKS; ++ch) {
    const V16 kv = *reinterpret_cast<const V16*>(Kp + ch * VN);
#pragma unroll
    for (int e = 0; e < VN; e += 2) {
      s0 = fmaf(q[ch * VN + e], to_f32(kv[e]), s0);
      s1 = fmaf(q[ch * VN + e + 1], to_f32(kv[e + 1]), s1);
    }
  }
  const float s = s0 + s1;
  if (s > mx) {
    const float alpha = __expf(mx - s);
    l *= alpha;
#pragma unroll
    for (int c = 0; c < HD; ++c) acc[c] *= alpha;
    mx = s;
  }
  const float p = __expf(s - mx);
  l += p;
#pragma unroll
  for (int ch = 0; ch < CHUNKS; ++ch) {
    const V16 vv = *reinterpret_cast<const V16*>(Vp + ch * VN);
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[ch * VN + e] = fmaf(p, to_f32(vv[e]), acc[ch * VN + e]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void attn_rows_kernel(const T* __restrict__ qkv, int64_t ld_qkv, T* __restrict__ out,
                                                        int64_t ld_out, int tokens, int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* Ks = reinterpret_cast<T*>(smem_raw);
  T* Vs = Ks + (size_t)tokens * HD;
  using V16 = typename Vec16<T>::type;
  constexpr int VN = Vec16<T>::N;
  constexpr int CHUNKS = HD / VN;  // 16-byte chunks per head row
  const int frame = blockIdx.x / heads, head = blockIdx.x % heads;
  const int D = heads * HD;
  const T* base = qkv + (int64_t)frame * tokens * ld_qkv + head * HD;

  for (int c = threadIdx.x; c < tokens * CHUNKS; c += blockDim.x) {
    const int row = c / CHUNKS, ch = c % CHUNKS;
    const T* src = base + (int64_t)row * ld_qkv + ch * VN;
    *reinterpret_cast<V16*>(Ks + row * HD + ch * VN) = *reinterpret_cast<const V16*>(src + D);
    *reinterpret_cast<V16*>(Vs + row * HD + ch * VN) = *reinterpret_cast<const V16*>(src + 2 * D);
  }
  __syncthreads();

  for (int qi = threadIdx.x; qi < tokens; qi += blockDim.x) {
    float q[HD], acc[HD];
    const T* qp = base + (int64_t)qi * ld_qkv;
#pragma unroll
    for (int ch = 0; ch < CHUNKS; ++ch) {
      const V16 v = *reinterpret_cast<const V16*>(qp + ch * VN);
#pragma unroll
      for (int e = 0; e < VN; ++e) q[ch * VN + e] = to_f32(v[e]) * scale;
    }
#pragma unroll
    for (int c = 0; c < HD; ++c) acc[c] = 0.f;
    float mx = -INFINITY, l = 0.f;
    for (int j = 0; j < tokens; ++j) {
      attn_row_key<T>(q, acc, mx, l, Ks + j * HD, Vs + j * HD);
    }
    const float inv = 1.0f / l;
    T* op = out + ((int64_t)frame * tokens + qi) * ld_out + head * HD;
#pragma unroll
    for (int ch = 0; ch < CHUNKS; ++ch) {
      V16 o;
#pragma unroll
      for (int e = 0; e < VN; ++e) o[e] = from_f32<T>(acc[ch * VN + e] * inv);
      *reinterpret_cast<V16*>(op + ch * VN) = o;
    }
  }
}

// K and V in chunks of `chunk` keys: every thread takes part in every refill, also where it has no query row.
template <typename T>
__global__ __launch_bounds__(256) void attn_rows_chunked_kernel(const T* __restrict__ qkv, int64_t ld_qkv, T* __restrict__ out,
                                                                int64_t ld_out, int tokens, int heads, float scale, int chunk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* Ks = reinterpret_cast<T*>(smem_raw);
  T* Vs = Ks + (size_t)chunk * HD;
  using V16 = typename Vec16<T>::type;
  constexpr int VN = Vec16<T>::N;
  constexpr int CHUNKS = HD / VN;
  const int frame = blockIdx.x / heads, head = blockIdx.x % heads;
  const int D = heads * HD;
  const T* base = qkv + (int64_t)frame * tokens * ld_qkv + head * HD;

  for (int qbase = 0; qbase < tokens; qbase += blockDim.x) {
    const int qi = qbase + threadIdx.x;
    const bool live = qi < tokens;
    float q[HD], acc[HD];
    const T* qp = base + (int64_t)(live ? qi : tokens - 1) * ld_qkv;
#pragma unroll
    for (int ch = 0; ch < CHUNKS; ++ch) {
      const V16 v = *reinterpret_cast<const V16*>(qp + ch * VN);
#pragma unroll
      for (int e = 0; e < VN; ++e) q[ch * VN + e] = to_f32(v[e]) * scale;
    }
#pragma unroll
    for (int c = 0; c < HD; ++c) acc[c] = 0.f;
    float mx = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < tokens; k0 += chunk) {
      const int nk = min(chunk, tokens - k0);
      __syncthreads();  // the previous chunk has been consumed
      for (int c = threadIdx.x; c < nk * CHUNKS; c += blockDim.x) {
        const int row = c / CHUNKS, ch = c % CHUNKS;
        const T* src = base + (int64_t)(k0 + row) * ld_qkv + ch * VN;
        *reinterpret_cast<V16*>(Ks + row * HD + ch * VN) = *reinterpret_cast<const V16*>(src + D);
        *reinterpret_cast<V16*>(Vs + row * HD + ch * VN) = *reinterpret_cast<const V16*>(src + 2 * D);
      }
      __syncthreads();
      if (live)
        for (int j = 0; j < nk; ++j) attn_row_key<T>(q, acc, mx, l, Ks + j * HD, Vs + j * HD);
    }
    if (live) {
      const float inv = 1.0f / l;
      T* op = out + ((int64_t)frame * tokens + qi) * ld_out + head * HD;
#pragma unroll
      for (int ch = 0; ch < CHUNKS; ++ch) {
        V16 o;
#pragma unroll
        for (int e = 0; e < VN; ++e) o[e] = from_f32<T>(acc[ch * VN + e] * inv);
        *reinterpret_cast<V16*>(op + ch * VN) = o;
      }
    }
  }
}

template <typename T>
int launch_rows(const AttnPlan& p, const AttnCall& c) {
  const T* qkv = static_cast<const T*>(c.qkv);
  T* out = static_cast<T*>(c.out);
  if (p.path == ATTN_ROWS_CHUNKED)
    return attn_launch<&attn_rows_chunked_kernel<T>>("dfd_attention_fwd", p, c.st, qkv, c.ld_qkv, out, c.ld_out, c.tokens, c.heads, c.scale, p.chunk);
  return attn_launch<&attn_rows_kernel<T>>("dfd_attention_fwd", p, c.st, qkv, c.ld_qkv, out, c.ld_out, c.tokens, c.heads, c.scale);
}

thread_local int g_attn_variant = 0;
thread_local int g_attn_last_path = 0;

// What dfd_attention_fwd refuses about a shape, and the plan for what it accepts.
int checked_plan(AttnPlan* p, int dtype, int n_frames, int tokens, int heads, int64_t ld_qkv, int64_t ld_out, int n_cu) {
  DFD_REQUIRE(n_frames >= 0 && tokens > 0 && heads > 0, "dfd_attention_fwd: bad shape");
  DFD_REQUIRE(dtype == DFD_F32 || dtype == DFD_BF16, "dfd_attention_fwd: dtype=%d", dtype);
  const int esz = dtype == DFD_F32 ? 4 : 2;
  DFD_REQUIRE(ld_qkv >= 3 * heads * HD && ld_out >= heads * HD && (ld_qkv * esz) % 16 == 0 && (ld_out * esz) % 16 == 0,
              "dfd_attention_fwd: bad leading dimensions");
  *p = attn_plan(dtype, n_frames, tokens, heads, ld_qkv, ld_out, g_attn_variant, n_cu > 0 ? n_cu : dfd_cu_count());
  DFD_REQUIRE(p->path != ATTN_NONE, "dfd_attention_fwd: %lld (frame, head) items do not fit a grid", (long long)n_frames * heads);
  return DFD_OK;
}

}  // namespace

// Test hooks (include/dfdclip_hooks.h, which also holds the selection table).  Variant: 0 = default, 1 = force the chunked
// staging of the rows kernel with 16-key chunks, 2 = skip the streaming MFMA kernel.  Per thread; returns the previous value.
extern "C" int dfd_attention_set_variant(int variant) {
  const int old = g_attn_variant;
  g_attn_variant = variant;
  return old;
}

extern "C" int dfd_attention_last_path(void) { return g_attn_last_path; }

extern "C" int dfd_attention_plan(int dtype, int n_frames, int tokens, int heads, int64_t ld_qkv, int64_t ld_out, int n_cu,
                                  dfd_attention_plan_t* out) {
  AttnPlan p;
  if (checked_plan(&p, dtype, n_frames, tokens, heads, ld_qkv, ld_out, n_cu) != DFD_OK) return -1;
  if (out) *out = dfd_attention_plan_t{p.path, p.grid, p.block, p.chunk, (uint64_t)p.lds};
  return p.path;
}

extern "C" int dfd_attention_fwd(const void* qkv, int64_t ld_qkv, void* out, int64_t ld_out, int dtype, int n_frames,
                                 int tokens, int heads, int head_dim, float scale, void* stream) {
  DFD_REQUIRE(qkv && out, "dfd_attention_fwd: null pointer");
  DFD_REQUIRE(head_dim == HD, "dfd_attention_fwd: head_dim=%d, only 64 is supported", head_dim);
  AttnPlan p;
  if (int rc = checked_plan(&p, dtype, n_frames, tokens, heads, ld_qkv, ld_out, 0)) return rc;
  DFD_REQUIRE(dfd_aligned16(qkv) && dfd_aligned16(out), "dfd_attention_fwd: pointers must be 16-byte aligned");
  if (n_frames == 0) return DFD_OK;
  const AttnCall c{qkv, ld_qkv, out, ld_out, n_frames, tokens, heads, scale, static_cast<hipStream_t>(stream)};
  int rc;
  switch (p.path) {
    case ATTN_ROWS:
    case ATTN_ROWS_CHUNKED: rc = dtype == DFD_F32 ? launch_rows<float>(p, c) : launch_rows<bf16_t>(p, c); break;
    case ATTN_XROW: rc = dfd_attn_launch_xrow(p, c); break;
    case ATTN_STREAM: rc = dfd_attn_launch_stream(p, c); break;
    default: rc = dfd_attn_launch_mfma(p, c); break;  // ATTN_ITEM7, ATTN_ITEM9, ATTN_PERSIST7_SHORT, ATTN_PERSIST7
  }
  if (rc == DFD_OK) g_attn_last_path = p.path;
  return rc;
}
