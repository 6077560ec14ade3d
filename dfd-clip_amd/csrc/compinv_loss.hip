// dfd_compinv_loss_fwd / _bwd — CompInvEncoder's pair loss (reference src/models.py:1017-1051) on the adapted K/V.
//
// Forward: one workgroup owns one row p' of M [P, D] and a tile of CW 16-byte column vectors.  Its 256 threads are
// CW column lanes x `slots` reduction lanes; reduction lane s walks the items (frame tl, pair i, layer l) with
// index j = s, s + slots, ... in that order (k before v inside an item) and keeps f32 sums of |A[2i] - A[2i+1]|
// over the T consecutive clip-local rows p'*T + tl.  The lanes are then added in LDS in slot order.  S is never
// written; every order is fixed by (T, w, L, D) alone, so the result does not depend on the launch and repeats
// bit for bit.  ||M||^2: per-workgroup partial sums (one wave's butterfly) into the workspace, then one workgroup
// adds them in index order (compinv_norm_kernel).
//
// Backward: elementwise over both members of every pair, 16-byte vectors; the odd last clip is zero-filled.
#include "common.hpp"

namespace {

constexpr int kBlock = 256;

template <typename T> struct Vec;
template <> struct Vec<float> {
  static constexpr int N = 4;
  typedef f32x4 type;
};
template <> struct Vec<bf16_t> {
  static constexpr int N = 8;
  typedef bf16x8 type;
};

// column vectors per workgroup: the fewest tiles of at most 64 vectors that divide NV evenly
static inline int col_tiles(int nv) {
  int n = (nv + 63) / 64;
  while (nv % n) ++n;
  return n;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void compinv_fwd_kernel(const T* __restrict__ k, const T* __restrict__ v, int Tf, int P,
                                                             int D, int L, int B, int cw, int slots, float* __restrict__ M,
                                                             float* __restrict__ partial) {
  constexpr int VEC = Vec<T>::N;
  typedef typename Vec<T>::type vec_t;
  __shared__ float red[kBlock * VEC];
  __shared__ float wsum[kBlock / DFD_WAVE];
  const int tid = threadIdx.x;
  const int lane = tid % cw, slot = tid / cw;
  const int prow = blockIdx.y;
  const int c0 = (blockIdx.x * cw + lane) * VEC;
  const int w = B / 2;
  const int64_t clip = (int64_t)Tf * P * D;  // elements of one clip in one layer slab
  const int64_t lstride = (int64_t)B * clip;
  float acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
  if (slot < slots) {
    const int items = Tf * w * L;
    for (int j = slot; j < items; j += slots) {
      const int l = j % L, q = j / L;
      const int i = q % w, tl = q / w;
      const int64_t off = (int64_t)l * lstride + (int64_t)(2 * i) * clip + ((int64_t)prow * Tf + tl) * D + c0;
      const vec_t ka = *reinterpret_cast<const vec_t*>(k + off), kb = *reinterpret_cast<const vec_t*>(k + off + clip);
      const vec_t va = *reinterpret_cast<const vec_t*>(v + off), vb = *reinterpret_cast<const vec_t*>(v + off + clip);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] += fabsf((float)ka[e] - (float)kb[e]);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] += fabsf((float)va[e] - (float)vb[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) red[tid * VEC + e] = acc[e];
  __syncthreads();
  float sq = 0.f;
  if (tid < cw) {  // slot 0: add the reduction lanes in slot order, scale, store a row segment of M
    float m[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) m[e] = red[tid * VEC + e];
    for (int s = 1; s < slots; ++s) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) m[e] += red[(s * cw + tid) * VEC + e];
    }
    const float div_pairs = (float)(w * L * 2), div_t = (float)Tf;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      m[e] = m[e] / div_pairs / div_t;
      sq += m[e] * m[e];
    }
    float* dst = M + (int64_t)prow * D + c0;
#pragma unroll
    for (int e = 0; e < VEC; e += 4) *reinterpret_cast<f32x4*>(dst + e) = f32x4{m[e], m[e + 1], m[e + 2], m[e + 3]};
  }
  // cw <= 64: every contributing thread is in wave 0
  if (tid < DFD_WAVE) {
    sq = wave_sum(sq);
    if (tid == 0) wsum[0] = sq;
  }
  __syncthreads();
  if (tid == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = wsum[0];
}

__global__ __launch_bounds__(kBlock) void compinv_norm_kernel(const float* __restrict__ partial, int n, int P,
                                                              float* __restrict__ match, float* __restrict__ norm,
                                                              float* __restrict__ recon) {
  __shared__ float wsum[kBlock / DFD_WAVE];
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int j = tid; j < n; j += kBlock) s += partial[j];
  s = wave_sum(s);
  if (tid % DFD_WAVE == 0) wsum[tid / DFD_WAVE] = s;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int q = 0; q < kBlock / DFD_WAVE; ++q) t += wsum[q];
    const float nr = sqrtf(t);
    *norm = nr;
    *match = nr / (float)P;
    if (recon) *recon = 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void compinv_bwd_kernel(const T* __restrict__ k, const T* __restrict__ v,
                                                             T* __restrict__ dk, T* __restrict__ dv,
                                                             const float* __restrict__ M, const float* __restrict__ norm,
                                                             const float* __restrict__ grad, int Tf, int P, int D, int L,
                                                             int w, int B, int nvec, FastDiv div_nv, FastDiv div_t) {
  constexpr int VEC = Vec<T>::N;
  typedef typename Vec<T>::type vec_t;
  const int e = blockIdx.x * kBlock + threadIdx.x;  // vector index inside one clip's [T*P, D] slab
  if (e >= nvec) return;
  const int slabs = w + (B & 1);
  const int l = blockIdx.y / slabs, i = blockIdx.y % slabs;
  const int r = (int)div_nv.div((uint32_t)e);
  const int c0 = (e - r * (D / VEC)) * VEC;
  const int64_t clip = (int64_t)Tf * P * D;
  const int64_t off = (int64_t)l * B * clip + (int64_t)(2 * i) * clip + (int64_t)r * D + c0;
  if (i == w) {  // the odd last clip takes no part in the loss
    vec_t z;
#pragma unroll
    for (int q = 0; q < VEC; ++q) z[q] = (T)0.f;
    *reinterpret_cast<vec_t*>(dk + off) = z;
    *reinterpret_cast<vec_t*>(dv + off) = z;
    return;
  }
  const float nr = *norm;
  // d match / d M = M / (||M|| * P); d M / d S = 1/T over the row's group; d S / d A = sign / (w*L*2)
  const float scale = nr > 0.f ? *grad / ((float)Tf * nr * (float)P * (float)(w * L * 2)) : 0.f;
  const float* mrow = M + (int64_t)div_t.div((uint32_t)r) * D + c0;
  float g[VEC];
#pragma unroll
  for (int q = 0; q < VEC; q += 4) {
    const f32x4 mv = *reinterpret_cast<const f32x4*>(mrow + q);
#pragma unroll
    for (int u = 0; u < 4; ++u) g[q + u] = mv[u] * scale;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const T* src = t ? v : k;
    T* dst = t ? dv : dk;
    const vec_t a = *reinterpret_cast<const vec_t*>(src + off), b = *reinterpret_cast<const vec_t*>(src + off + clip);
    vec_t da, db;
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      const float x = (float)a[q], y = (float)b[q];
      const float d = (x > y ? g[q] : (x < y ? -g[q] : 0.f));
      da[q] = (T)d;
      db[q] = (T)(-d);
    }
    *reinterpret_cast<vec_t*>(dst + off) = da;
    *reinterpret_cast<vec_t*>(dst + off + clip) = db;
  }
}

int check_shape(const char* name, int dtype, int B, int T, int P, int D, int L) {
  DFD_REQUIRE(dtype == DFD_F32 || dtype == DFD_BF16, "%s: dtype must be f32 or bf16", name);
  DFD_REQUIRE(B >= 2, "%s: needs at least one pair of clips (B >= 2), got B = %d", name, B);
  DFD_REQUIRE(T >= 1 && P >= 1 && L >= 1 && D >= 8 && D % 8 == 0, "%s: bad shape T=%d P=%d D=%d L=%d", name, T, P, D, L);
  DFD_REQUIRE((int64_t)T * P * (D / 4) < (1ll << 31), "%s: one clip's slab is too large", name);
  return DFD_OK;
}

}  // namespace

extern "C" size_t dfd_compinv_loss_workspace(int P, int D) {
  if (P < 1 || D < 8 || D % 8) return 0;
  // M [P, D], then one partial sum per forward workgroup (for either dtype's tiling)
  const int tiles = col_tiles(D / 4) > col_tiles(D / 8) ? col_tiles(D / 4) : col_tiles(D / 8);
  return ((size_t)P * D + (size_t)P * tiles) * sizeof(float);
}

extern "C" int dfd_compinv_loss_fwd(const void* k, const void* v, int dtype, int B, int T, int P, int D, int L, void* workspace,
                                    float* match, float* norm, float* recon, void* stream) {
  DFD_REQUIRE(k && v && workspace && match && norm, "dfd_compinv_loss_fwd: null pointer");
  if (int rc = check_shape("dfd_compinv_loss_fwd", dtype, B, T, P, D, L)) return rc;
  DFD_REQUIRE(dfd_aligned16(k) && dfd_aligned16(v) && dfd_aligned16(workspace), "dfd_compinv_loss_fwd: buffers must be 16-byte aligned");
  const int vec = dtype == DFD_F32 ? 4 : 8;
  const int nv = D / vec, tiles = col_tiles(nv), cw = nv / tiles, slots = kBlock / cw;
  float* M = static_cast<float*>(workspace);
  float* partial = M + (size_t)P * D;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(tiles, P), block(kBlock);
  if (dtype == DFD_F32)
    hipLaunchKernelGGL(compinv_fwd_kernel<float>, grid, block, 0, st, static_cast<const float*>(k), static_cast<const float*>(v),
                       T, P, D, L, B, cw, slots, M, partial);
  else
    hipLaunchKernelGGL(compinv_fwd_kernel<bf16_t>, grid, block, 0, st, static_cast<const bf16_t*>(k),
                       static_cast<const bf16_t*>(v), T, P, D, L, B, cw, slots, M, partial);
  DFD_CHECK_LAUNCH("dfd_compinv_loss_fwd");
  hipLaunchKernelGGL(compinv_norm_kernel, dim3(1), block, 0, st, partial, tiles * P, P, match, norm, recon);
  DFD_CHECK_LAUNCH("dfd_compinv_loss_fwd (norm)");
  return DFD_OK;
}

extern "C" int dfd_compinv_loss_bwd(const void* k, const void* v, int dtype, int B, int T, int P, int D, int L, const void* workspace,
                                    const float* norm, const float* grad, void* dk, void* dv, void* stream) {
  DFD_REQUIRE(k && v && workspace && norm && grad && dk && dv, "dfd_compinv_loss_bwd: null pointer");
  if (int rc = check_shape("dfd_compinv_loss_bwd", dtype, B, T, P, D, L)) return rc;
  DFD_REQUIRE(dfd_aligned16(k) && dfd_aligned16(v) && dfd_aligned16(dk) && dfd_aligned16(dv) && dfd_aligned16(workspace),
              "dfd_compinv_loss_bwd: buffers must be 16-byte aligned");
  const int vec = dtype == DFD_F32 ? 4 : 8;
  const int nvec = T * P * (D / vec);
  const int w = B / 2, slabs = w + (B & 1);
  DFD_REQUIRE((int64_t)L * slabs < 65536, "dfd_compinv_loss_bwd: too many (layer, pair) slabs");
  const FastDiv div_nv = FastDiv::make((uint32_t)(D / vec)), div_t = FastDiv::make((uint32_t)T);
  const float* M = static_cast<const float*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((nvec + kBlock - 1) / kBlock, L * slabs), block(kBlock);
  if (dtype == DFD_F32)
    hipLaunchKernelGGL(compinv_bwd_kernel<float>, grid, block, 0, st, static_cast<const float*>(k), static_cast<const float*>(v),
                       static_cast<float*>(dk), static_cast<float*>(dv), M, norm, grad, T, P, D, L, w, B, nvec, div_nv, div_t);
  else
    hipLaunchKernelGGL(compinv_bwd_kernel<bf16_t>, grid, block, 0, st, static_cast<const bf16_t*>(k),
                       static_cast<const bf16_t*>(v), static_cast<bf16_t*>(dk), static_cast<bf16_t*>(dv), M, norm, grad, T, P, D,
                       L, w, B, nvec, div_nv, div_t);
  DFD_CHECK_LAUNCH("dfd_compinv_loss_bwd");
  return DFD_OK;
}
