// CompInvAdapter structs without a LayerNorm (reference src/models.py:877-922):
//   "768-bn"       kv + Dropout_p(BatchNorm2d(T)(kv · W0ᵀ))            channel = frame index t, statistics over (b, p, 768)
//   "768-xxx-768"  kv + Dropout_p(W6 · drop(GELU(W3 · drop(GELU(W0 · kv)))))
//   "linear"       Dropout_p(kv · W0ᵀ)                                  no residual
// The GEMMs are dfd_gemm / dfd_gemm_at_b; this file holds the elementwise and reduction stages between them.
//
// BatchNorm statistics are deterministic: every block writes (count, mean, M2) of its 8192-element chunk of one frame
// to a workspace slab, and one wave per channel merges a channel's partials in a fixed order (Chan's parallel update;
// no float atomics, no E[y²] - E[y]², which cancels at the 2.4 M values of a channel at B16xT30).  The backward's two
// sums (Σdz, Σdz·ŷ) take the same partial-slab route.  All streaming kernels move 16 bytes per lane per access.
#include "adapter_common.hpp"
#include "dropout.hpp"
#include "gelu.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kIters = 4;                          // 16-byte loads per thread per chunk
constexpr int kChunk = kThreads * 8 * kIters;      // elements of one frame a statistics block covers

// gelu_erf / gelu_erf_grad: gelu.hpp (shared with the GEMM epilogue)

// (n, mean, M2) of a set, merged with another (Chan et al.); n = 0 on either side is the identity
struct Moments {
  float n, mean, m2;
};
__device__ __forceinline__ Moments merge(Moments a, Moments b) {
  const float n = a.n + b.n;
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  const float d = b.mean - a.mean, f = b.n / n;
  return Moments{n, fmaf(d, f, a.mean), a.m2 + b.m2 + d * d * a.n * f};
}
__device__ __forceinline__ Moments wave_merge(Moments m) {  // fixed butterfly: lane 0 ends with the same bits every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    m = merge(m, Moments{__shfl_xor(m.n, o, 64), __shfl_xor(m.mean, o, 64), __shfl_xor(m.m2, o, 64)});
  return m;
}

// ---- statistics, pass 1: block (frame f, chunk c) -> part[f * chunks + c] = {n, mean, M2} ---------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void bn_partial_kernel(const T* __restrict__ y, float* __restrict__ part, int slab,
                                                              int chunks) {
  __shared__ float sh[3][kThreads / 64];
  const int f = blockIdx.x / chunks, c = blockIdx.x - f * chunks;
  const T* base = y + (int64_t)f * slab;
  float v[kIters][8];
  int nv = 0;
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = c * kChunk + (it * kThreads + (int)threadIdx.x) * 8;
    if (i < slab) {  // slab % 8 == 0: a vector is whole or absent
      Vec<T, 8>::load(base + i, v[it]);
      nv += 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[it][e];
    }
  }
  Moments m{(float)nv, nv ? s / (float)nv : 0.f, 0.f};
#pragma unroll
  for (int it = 0; it < kIters; ++it)
    if (c * kChunk + (it * kThreads + (int)threadIdx.x) * 8 < slab) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[it][e] - m.mean; m.m2 = fmaf(d, d, m.m2); }
    }
  m = wave_merge(m);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[0][wave] = m.n; sh[1][wave] = m.mean; sh[2][wave] = m.m2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    Moments t{sh[0][0], sh[1][0], sh[2][0]};
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) t = merge(t, Moments{sh[0][w], sh[1][w], sh[2][w]});
    float* o = part + (int64_t)blockIdx.x * 4;
    *reinterpret_cast<f32x4*>(o) = f32x4{t.n, t.mean, t.m2, 0.f};
  }
}

// ---- statistics, pass 2: one wave per channel t merges the partials of frames t, t+T, ... in a fixed order ----------
// mode 0: eval (mean / invstd from the running statistics, y unread); 1: batch statistics; 2: also update running.
__global__ __launch_bounds__(64) void bn_merge_kernel(const float* __restrict__ part, float* __restrict__ stats,
                                                      float* __restrict__ running_mean, float* __restrict__ running_var,
                                                      int64_t* __restrict__ num_batches_tracked, int clips, int T,
                                                      int chunks, int mode, float momentum, float eps) {
  const int t = blockIdx.x, lane = threadIdx.x;
  if (mode == 0) {
    if (lane == 0) {
      stats[t] = running_mean[t];
      stats[T + t] = 1.0f / sqrtf(running_var[t] + eps);
    }
    return;
  }
  Moments m{0.f, 0.f, 0.f};
  const int np = clips * chunks;
  for (int j = lane; j < np; j += 64) {
    const int b = j / chunks, c = j - b * chunks;
    const f32x4 p = *reinterpret_cast<const f32x4*>(part + ((int64_t)(b * T + t) * chunks + c) * 4);
    m = merge(m, Moments{p[0], p[1], p[2]});
  }
  m = wave_merge(m);
  if (lane == 0) {
    const float var = m.m2 / m.n;  // biased: what normalises (nn.BatchNorm2d in train mode)
    stats[t] = m.mean;
    stats[T + t] = 1.0f / sqrtf(var + eps);
    if (mode == 2) {
      running_mean[t] = (1.0f - momentum) * running_mean[t] + momentum * m.mean;
      running_var[t] = (1.0f - momentum) * running_var[t] + momentum * (var * (m.n / (m.n - 1.0f)));
      if (t == 0) num_batches_tracked[0] += 1;
    }
  }
}

// ---- apply: out = residual + drop(γ_t (y - μ_t) invstd_t + β_t) + pos[t]   (stats == NULL: drop(y) + pos) ----------
template <typename TY, typename T>
__global__ __launch_bounds__(kThreads) void bn_apply_kernel(const TY* y, const T* residual, T* out,
                                                            const float* __restrict__ stats, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ pos,
                                                            int64_t groups, FastDiv row_div, FastDiv frame_div, int width,
                                                            int T_, DfdDrop drop) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
    const uint32_t row = row_div.div((uint32_t)g);
    const int col = (int)(g - (int64_t)row * (width >> 3)) * 8;
    const int t = (int)(frame_div.div(row) % (uint32_t)T_);
    const int64_t e0 = g * 8;
    float v[8];
    Vec<TY, 8>::load(y + e0, v);
    if (stats != nullptr) {
      const float mu = stats[t], is = stats[T_ + t], ga = gamma[t], be = beta[t];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = ga * ((v[e] - mu) * is) + be;
    }
    dfd_drop_eight(drop, (uint64_t)e0, v);
    float r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (residual != nullptr) Vec<T, 8>::load(residual + e0, r);
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (pos != nullptr) Vec<float, 8>::load(pos + (int64_t)t * width + col, p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = r[e] + v[e] + p[e];
    Vec<T, 8>::store(out + e0, v);
  }
}

// ---- backward, pass 1: block (frame, chunk) -> part = {Σdz, Σdz·ŷ}, dz = mask·dOut, ŷ = (y - μ) invstd -------------
template <typename T, typename TD>
__global__ __launch_bounds__(kThreads) void bn_bwd_partial_kernel(const T* __restrict__ y, const TD* __restrict__ dout,
                                                                  const float* __restrict__ stats, float* __restrict__ part,
                                                                  int slab, int chunks, int T_, DfdDrop drop) {
  __shared__ float sh[2][kThreads / 64];
  const int f = blockIdx.x / chunks, c = blockIdx.x - f * chunks;
  const int t = f % T_;
  const float mu = stats[t], is = stats[T_ + t];
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int it = 0; it < kIters; ++it) {
    const int i = c * kChunk + (it * kThreads + (int)threadIdx.x) * 8;
    if (i < slab) {
      const int64_t e0 = (int64_t)f * slab + i;
      float yv[8], dz[8];
      Vec<T, 8>::load(y + e0, yv);
      Vec<TD, 8>::load(dout + e0, dz);
      dfd_drop_eight(drop, (uint64_t)e0, dz);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s0 += dz[e];
        s1 = fmaf(dz[e], (yv[e] - mu) * is, s1);
      }
    }
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[0][wave] = s0; sh[1][wave] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) { a += sh[0][w]; b += sh[1][w]; }
    float* o = part + (int64_t)blockIdx.x * 4;
    *reinterpret_cast<f32x4*>(o) = f32x4{a, b, 0.f, 0.f};
  }
}

// ---- backward, pass 2: one wave per channel: dβ_t = Σdz, dγ_t = Σdz·ŷ (fixed order) -------------------------------
__global__ __launch_bounds__(64) void bn_bwd_merge_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta, int clips, int T, int chunks) {
  const int t = blockIdx.x, lane = threadIdx.x;
  float s0 = 0.f, s1 = 0.f;
  const int np = clips * chunks;
  for (int j = lane; j < np; j += 64) {
    const int b = j / chunks, c = j - b * chunks;
    const f32x4 p = *reinterpret_cast<const f32x4*>(part + ((int64_t)(b * T + t) * chunks + c) * 4);
    s0 += p[0];
    s1 += p[1];
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (lane == 0) {
    dbeta[t] = s0;
    dgamma[t] = s1;
  }
}

// ---- backward, pass 3: dy = γ invstd (dz - Σdz/n - ŷ Σdzŷ/n)  (train)  |  γ invstd dz  (eval) ---------------------
template <typename T, typename TD>
__global__ __launch_bounds__(kThreads) void bn_bwd_apply_kernel(const T* y, const TD* dout, T* dy, const float* __restrict__ stats,
                                                                const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                                const float* __restrict__ dbeta, int64_t groups, FastDiv frame_div,
                                                                int T_, float inv_n, int train, DfdDrop drop) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
    const int t = (int)(frame_div.div((uint32_t)g) % (uint32_t)T_);  // frame_div divides by slab / 8
    const int64_t e0 = g * 8;
    const float mu = stats[t], is = stats[T_ + t], k = gamma[t] * is;
    const float mb = train ? dbeta[t] * inv_n : 0.f, mg = train ? dgamma[t] * inv_n : 0.f;
    float yv[8], dz[8];
    Vec<T, 8>::load(y + e0, yv);
    Vec<TD, 8>::load(dout + e0, dz);
    dfd_drop_eight(drop, (uint64_t)e0, dz);
#pragma unroll
    for (int e = 0; e < 8; ++e) yv[e] = k * (dz[e] - mb - ((yv[e] - mu) * is) * mg);
    Vec<T, 8>::store(dy + e0, yv);
  }
}

// ---- GELU (erf form, nn.GELU()) with the following dropout fused: out = drop(GELU(a));  backward: da = GELU'(a)·drop(dh)
template <typename TA, typename TH, typename TO>
__global__ __launch_bounds__(kThreads) void gelu_erf_kernel(const TA* __restrict__ a, const TH* __restrict__ dh,
                                                            TO* __restrict__ out, int64_t groups, DfdDrop drop) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += stride) {
    const int64_t e0 = g * 8;
    float v[8];
    Vec<TA, 8>::load(a + e0, v);
    if (dh == nullptr) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = gelu_erf(v[e]);
      dfd_drop_eight(drop, (uint64_t)e0, v);
    } else {
      float d[8];
      Vec<TH, 8>::load(dh + e0, d);
      dfd_drop_eight(drop, (uint64_t)e0, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = gelu_erf_grad(v[e]) * d[e];
    }
    Vec<TO, 8>::store(out + e0, v);
  }
}

unsigned stream_grid(int64_t groups) {  // grid-stride: at most 8 blocks of 256 per CU of a 256-CU part
  const int64_t b = (groups + kThreads - 1) / kThreads;
  return (unsigned)(b < 2048 ? (b > 0 ? b : 1) : 2048);
}


int chunks_of(int64_t slab) { return (int)((slab + kChunk - 1) / kChunk); }

// What dfd_adapter_bn_apply and dfd_adapter_bn_bwd ask alike of the tensor and of the buffers they move 16 bytes at a time;
// the backward also needs whole clips (frames > 0, a multiple of T).
int bn_check(const char* fn, int64_t frames, int patches, int width, int T, bool backward, std::initializer_list<const void*> bufs) {
  DFD_REQUIRE(T > 0 && frames >= (backward ? 1 : 0) && patches > 0 && width > 0 && (!backward || frames % T == 0) && width % 8 == 0,
              "%s: bad shape", fn);
  DFD_REQUIRE(frames * patches * width < (1ll << 31), "%s: tensor of 2^31 elements or more", fn);
  for (const void* p : bufs) DFD_REQUIRE(dfd_aligned16(p), "%s: buffers must be 16-byte aligned", fn);
  return DFD_OK;
}

// What dfd_gelu_erf and dfd_gelu_erf_bwd ask alike: whole groups of 8 and 16-byte aligned buffers.
int gelu_check(const char* fn, int64_t n, std::initializer_list<const void*> bufs) {
  DFD_REQUIRE(n >= 0 && n % 8 == 0, "%s: n=%lld must be a multiple of 8", fn, (long long)n);
  for (const void* p : bufs) DFD_REQUIRE(dfd_aligned16(p), "%s: buffers must be 16-byte aligned", fn);
  return DFD_OK;
}

}  // namespace

extern "C" size_t dfd_adapter_bn_workspace(int64_t frames, int patches, int width) {
  if (frames <= 0 || patches <= 0 || width <= 0) return 0;
  return (size_t)frames * chunks_of((int64_t)patches * width) * 4 * sizeof(float);
}

extern "C" int dfd_adapter_bn_stats(const void* y, int dtype, float* stats, float* running_mean, float* running_var,
                                    int64_t* num_batches_tracked, void* workspace, int64_t frames, int patches, int width,
                                    int T, int mode, float momentum, float eps, void* stream) {
  DFD_REQUIRE(stats, "dfd_adapter_bn_stats: null pointer");
  DFD_REQUIRE(mode >= 0 && mode <= 2, "dfd_adapter_bn_stats: mode=%d", mode);
  DFD_REQUIRE(T > 0 && frames > 0 && patches > 0 && width > 0 && frames % T == 0, "dfd_adapter_bn_stats: bad shape");
  DFD_REQUIRE((int64_t)patches * width % 8 == 0 && frames * patches * width < (1ll << 31),
              "dfd_adapter_bn_stats: patches*width must be a multiple of 8 and the tensor below 2^31 elements");
  DFD_REQUIRE(mode == 1 || (running_mean && running_var), "dfd_adapter_bn_stats: mode %d needs the running statistics", mode);
  DFD_REQUIRE(mode != 2 || num_batches_tracked, "dfd_adapter_bn_stats: mode 2 needs num_batches_tracked");
  DFD_REQUIRE(mode == 0 || (y && workspace && dfd_aligned16(y) && dfd_aligned16(workspace)),
              "dfd_adapter_bn_stats: y / workspace null or not 16-byte aligned");
  DFD_REQUIRE(mode != 2 || frames / T * patches * width > 1, "dfd_adapter_bn_stats: one value per channel has no unbiased variance");
  DFD_REQUIRE(mode == 0 || ok_dtype(dtype), "dfd_adapter_bn_stats: dtype=%d", dtype);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slab = patches * width, chunks = chunks_of(slab);
  float* part = static_cast<float*>(workspace);
  if (mode != 0) {
    const dim3 grid((unsigned)(frames * chunks));
    if (dtype == DFD_F32)
      hipLaunchKernelGGL(bn_partial_kernel<float>, grid, dim3(kThreads), 0, st, static_cast<const float*>(y), part, slab, chunks);
    else
      hipLaunchKernelGGL(bn_partial_kernel<bf16_t>, grid, dim3(kThreads), 0, st, static_cast<const bf16_t*>(y), part, slab, chunks);
  }
  hipLaunchKernelGGL(bn_merge_kernel, dim3(T), dim3(64), 0, st, part, stats, running_mean, running_var, num_batches_tracked,
                     (int)(frames / T), T, chunks, mode, momentum, eps);
  DFD_CHECK_LAUNCH("dfd_adapter_bn_stats");
  return DFD_OK;
}

extern "C" int dfd_adapter_bn_apply(const void* y, int y_dtype, const void* residual, void* out, int dtype, const float* stats,
                                    const float* gamma, const float* beta, const float* pos, const dfd_dropout_t* drop,
                                    int64_t frames, int patches, int width, int T, void* stream) {
  const char* fn = "dfd_adapter_bn_apply";
  DFD_REQUIRE(y && out, "%s: null pointer", fn);
  DFD_REQUIRE(!stats || (gamma && beta), "%s: stats need gamma and beta", fn);
  DFD_REQUIRE(ok_dtype(y_dtype) && ok_dtype(dtype), "%s: dtypes %d / %d", fn, y_dtype, dtype);
  if (int rc = bn_check(fn, frames, patches, width, T, false, {y, out, residual, pos})) return rc;
  DFD_REQUIRE(y != out || y_dtype == dtype, "%s: in place on y needs one dtype", fn);
  if (int rc = check_drop(fn, drop)) return rc;
  if (frames == 0) return DFD_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t groups = frames * patches * width / 8;
  const FastDiv rd = FastDiv::make((uint32_t)(width / 8)), fd = FastDiv::make((uint32_t)patches);
  const DfdDrop d = dfd_make_drop(drop);
  with_types(y_dtype, dtype, [&](auto ty, auto t) {
    using TY = typename decltype(ty)::type;
    using T_ = typename decltype(t)::type;
    hipLaunchKernelGGL((bn_apply_kernel<TY, T_>), dim3(stream_grid(groups)), dim3(kThreads), 0, st, static_cast<const TY*>(y),
                       static_cast<const T_*>(residual), static_cast<T_*>(out), stats, gamma, beta, pos, groups, rd, fd, width, T, d);
  });
  DFD_CHECK_LAUNCH(fn);
  return DFD_OK;
}

extern "C" int dfd_adapter_bn_bwd(const void* y, const void* dout, int dout_dtype, void* dy, int dtype, const float* stats,
                                  const float* gamma, float* dgamma, float* dbeta, const dfd_dropout_t* drop, void* workspace,
                                  int64_t frames, int patches, int width, int T, int train, void* stream) {
  const char* fn = "dfd_adapter_bn_bwd";
  DFD_REQUIRE(y && dout && dy && stats && gamma && dgamma && dbeta && workspace, "%s: null pointer", fn);
  DFD_REQUIRE(ok_dtype(dtype) && (dout_dtype == dtype || dout_dtype == DFD_F32), "%s: dtypes %d / %d", fn, dtype, dout_dtype);
  if (int rc = bn_check(fn, frames, patches, width, T, true, {y, dout, dy, workspace})) return rc;
  if (int rc = check_drop(fn, drop)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slab = patches * width, chunks = chunks_of(slab), clips = (int)(frames / T);
  const int64_t groups = frames * slab / 8;
  float* part = static_cast<float*>(workspace);
  const FastDiv fd = FastDiv::make((uint32_t)(slab / 8));
  const float inv_n = 1.0f / ((float)clips * (float)slab);
  const DfdDrop d = dfd_make_drop(drop);
  with_types<false>(dout_dtype, dtype, [&](auto td, auto t) {  // dout is in dtype or f32
    using TD = typename decltype(td)::type;
    using T_ = typename decltype(t)::type;
    hipLaunchKernelGGL((bn_bwd_partial_kernel<T_, TD>), dim3((unsigned)(frames * chunks)), dim3(kThreads), 0, st,
                       static_cast<const T_*>(y), static_cast<const TD*>(dout), stats, part, slab, chunks, T, d);
    hipLaunchKernelGGL(bn_bwd_merge_kernel, dim3(T), dim3(64), 0, st, part, dgamma, dbeta, clips, T, chunks);
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T_, TD>), dim3(stream_grid(groups)), dim3(kThreads), 0, st, static_cast<const T_*>(y),
                       static_cast<const TD*>(dout), static_cast<T_*>(dy), stats, gamma, dgamma, dbeta, groups, fd, T, inv_n, train, d);
  });
  DFD_CHECK_LAUNCH(fn);
  return DFD_OK;
}

extern "C" int dfd_gelu_erf(const void* a, int a_dtype, void* out, int out_dtype, int64_t n, const dfd_dropout_t* drop,
                            void* stream) {
  const char* fn = "dfd_gelu_erf";
  DFD_REQUIRE(a && out, "%s: null pointer", fn);
  DFD_REQUIRE(ok_dtype(a_dtype) && ok_dtype(out_dtype), "%s: dtypes %d / %d", fn, a_dtype, out_dtype);
  if (int rc = gelu_check(fn, n, {a, out})) return rc;
  DFD_REQUIRE(a != out || a_dtype == out_dtype, "%s: in place needs one dtype", fn);
  if (int rc = check_drop(fn, drop)) return rc;
  if (n == 0) return DFD_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DfdDrop d = dfd_make_drop(drop);
  const int64_t groups = n / 8;
  with_types(a_dtype, out_dtype, [&](auto ta, auto to) {
    using TA = typename decltype(ta)::type;
    using TO = typename decltype(to)::type;
    hipLaunchKernelGGL((gelu_erf_kernel<TA, TA, TO>), dim3(stream_grid(groups)), dim3(kThreads), 0, st, static_cast<const TA*>(a),
                       static_cast<const TA*>(nullptr), static_cast<TO*>(out), groups, d);
  });
  DFD_CHECK_LAUNCH(fn);
  return DFD_OK;
}

extern "C" int dfd_gelu_erf_bwd(const void* a, int a_dtype, const void* dh, int dh_dtype, void* da, int da_dtype, int64_t n,
                                const dfd_dropout_t* drop, void* stream) {
  const char* fn = "dfd_gelu_erf_bwd";
  DFD_REQUIRE(a && dh && da, "%s: null pointer", fn);
  DFD_REQUIRE(ok_dtype(a_dtype) && ok_dtype(dh_dtype) && ok_dtype(da_dtype) && dh_dtype == da_dtype,
              "%s: dtypes %d / %d / %d (dh and da must agree)", fn, a_dtype, dh_dtype, da_dtype);
  if (int rc = gelu_check(fn, n, {a, dh, da})) return rc;
  DFD_REQUIRE(da != a || a_dtype == da_dtype, "%s: in place on a needs one dtype", fn);
  if (int rc = check_drop(fn, drop)) return rc;
  if (n == 0) return DFD_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DfdDrop d = dfd_make_drop(drop);
  const int64_t groups = n / 8;
  with_types(a_dtype, da_dtype, [&](auto ta, auto t) {
    using TA = typename decltype(ta)::type;
    using T_ = typename decltype(t)::type;
    hipLaunchKernelGGL((gelu_erf_kernel<TA, T_, T_>), dim3(stream_grid(groups)), dim3(kThreads), 0, st, static_cast<const TA*>(a),
                       static_cast<const T_*>(dh), static_cast<T_*>(da), groups, d);
  });
  DFD_CHECK_LAUNCH(fn);
  return DFD_OK;
}
