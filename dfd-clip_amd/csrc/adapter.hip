// CompInvAdapter middle stage (reference src/models.py:823-875): y = GELU_erf(LayerNorm(a)) over a
// [frames, patches, x] tensor.  "nln" normalises the whole (patches, x) slab of a frame jointly with a
// [patches, x] affine (models.py:831); "ln"/"z0" normalise each row of x (models.py:847, :860).
// HBM-bound: one read and one write of the tensor (slab kept in registers between the passes when it
// fits; the statistics pass re-reads from L2 otherwise).  fp32 statistics, two-pass variance.
//
// Device side: three statistics fronts (adp_strided_stats, adp_slab_stats, adp_row256_stats: they differ in arithmetic
// and stay apart) and the backward's dz term (adp_dz).  Host side: one call description (AdpCall), one argument check
// (adp_check), one plan (adp_plan: which kernel, which grid) and one launch function per direction.
#include "adapter_common.hpp"

#include "../../include/dfdclip_hooks.h"

namespace {

// The erff form of GELU and its derivative.  gelu.hpp's gelu_erf / gelu_erf_grad (adapter_structs.hip, the GEMM epilogue)
// go through dfd_norm_cdf and give other bits; this file's results are pinned to the erff form, so there are two.
__device__ __forceinline__ float adp_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float adp_gelu_grad(float z) {
  return 0.5f * (1.0f + erff(z * 0.70710678118654752f)) + z * 0.3989422804014327f * __expf(-0.5f * z * z);
}

template <typename T> __device__ __forceinline__ float ld(const T* p) { return to_f32(*p); }

// The normalised quantity at element i.  gelu_first ("768-x-768" / "legacy-768-x-768", models.py:795-821):
// y = LayerNorm(GELU(a)), so u = GELU(a) is what the statistics see; else GELU(LayerNorm(a)) and it is a itself.
template <typename TA> __device__ __forceinline__ float adp_in(const TA* ap, int64_t i, int gelu_first) {
  const float v = ld(ap + i);
  return gelu_first ? adp_gelu(v) : v;
}

struct AdpStats {
  float mean, rstd;
};

// Strided front: a thread takes elements first, first + stride, ... of the n at ap; `sum` adds across the threads that
// share the group (a wave or the workgroup).  Adds in stride order, divides by n; the elements are read twice.
template <typename TA, typename Stride, typename Sum>
__device__ __forceinline__ AdpStats adp_strided_stats(const TA* ap, int gelu_first, int first, Stride stride, int n, float eps, Sum&& sum) {
  float s = 0.f;
  for (int i = first; i < n; i += stride) s += adp_in(ap, i, gelu_first);
  const float mean = sum(s) / (float)n;
  float q = 0.f;
  for (int i = first; i < n; i += stride) { const float d = adp_in(ap, i, gelu_first) - mean; q += d * d; }
  return AdpStats{mean, rsqrtf(sum(q) / (float)n + eps)};
}

// Register-resident front of a 1024-thread workgroup: thread tid loads chunks tid, tid + 1024, ... of 8 elements (at most
// NCH of them, n % 8 == 0) into v ONCE and takes both statistics passes from the registers.
template <typename TA, int NCH>
__device__ __forceinline__ AdpStats adp_slab_stats(const TA* ap, int n, float eps, float (&v)[NCH][8], float* sc) {
  const int tid = threadIdx.x, nchunk = n >> 3;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = tid + c * 1024;
    if (ch < nchunk) {
      Vec<TA, 8>::load(ap + (int64_t)ch * 8, v[c]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[c][e];
    }
  }
  const float mean = block_sum<16>(s, sc) / (float)n;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    if (tid + c * 1024 < nchunk) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[c][e] - mean; q += d * d; }
    }
  return AdpStats{mean, rsqrtf(block_sum<16>(q, sc) / (float)n + eps)};
}

// Front of a 256-wide row held by one wave, 4 elements per lane: pairwise sum, times 1/256 (not the strided front's bits).
__device__ __forceinline__ AdpStats adp_row256_stats(const float (&v)[4], float eps) {
  const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / 256.0f);
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { const float d = v[e] - mean; q += d * d; }
  return AdpStats{mean, rsqrtf(wave_sum(q) * (1.0f / 256.0f) + eps)};
}

// Backward: dL/dz at the affine's output z = nhat * w + b.  The LayerNorm's incoming gradient is g = adp_dz(..) * w.
__device__ __forceinline__ float adp_dz(float dy, float nh, float w, float b, int gelu_first) {
  return dy * (gelu_first ? 1.0f : adp_gelu_grad(nh * w + b));
}

// one workgroup per frame (joint) — slab = patches * x elements
template <typename TA, typename T>
__global__ __launch_bounds__(1024) void adapter_nln_kernel(const TA* __restrict__ a, T* __restrict__ y,
                                                           const float* __restrict__ w, const float* __restrict__ b,
                                                           int slab, float eps) {
  __shared__ float sc[16];
  const int tid = threadIdx.x;
  const TA* ap = a + (int64_t)blockIdx.x * slab;
  T* yp = y + (int64_t)blockIdx.x * slab;
  const auto [mean, rstd] = adp_strided_stats(ap, 0, tid, blockDim.x, slab, eps, [&](float v) { return block_sum(v, sc); });
  for (int i = tid; i < slab; i += blockDim.x) yp[i] = from_f32<T>(adp_gelu((ld(ap + i) - mean) * rstd * w[i] + b[i]));
}

// Register-resident form of the joint ("nln") kernel: the frame's (patches, x) slab is read ONCE, 8
// elements (16 bytes of bf16) per load, held in registers across the two statistics passes and the
// affine + GELU pass.  Needs slab % 8 == 0 and slab <= 1024 * 8 * NCH.
template <typename TA, typename T, int NCH>
__global__ __launch_bounds__(1024) void adapter_nln_reg_kernel(const TA* __restrict__ a, T* __restrict__ y,
                                                               const float* __restrict__ w, const float* __restrict__ b,
                                                               int slab, float eps) {
  __shared__ float sc[16];
  const int tid = threadIdx.x, nchunk = slab >> 3;
  T* yp = y + (int64_t)blockIdx.x * slab;
  float v[NCH][8];
  const auto [mean, rstd] = adp_slab_stats<TA, NCH>(a + (int64_t)blockIdx.x * slab, slab, eps, v, sc);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = tid + c * 1024;
    if (ch < nchunk) {
      float ww[8], bb[8], o[8];
      Vec<float, 8>::load(w + (int64_t)ch * 8, ww);
      Vec<float, 8>::load(b + (int64_t)ch * 8, bb);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = adp_gelu((v[c][e] - mean) * rstd * ww[e] + bb[e]);
      Vec<T, 8>::store(yp + (int64_t)ch * 8, o);
    }
  }
}

// one wave per row of x
template <typename TA, typename T>
__global__ __launch_bounds__(256) void adapter_ln_kernel(const TA* __restrict__ a, T* __restrict__ y, const float* __restrict__ w,
                                                         const float* __restrict__ b, int64_t rows, int x, float eps,
                                                         int gelu_first) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const TA* ap = a + row * x;
  T* yp = y + row * x;
  const auto [mean, rstd] = adp_strided_stats(ap, gelu_first, lane, 64, x, eps, [](float v) { return wave_sum(v); });
  for (int i = lane; i < x; i += 64) {
    const float z = (adp_in(ap, i, gelu_first) - mean) * rstd * w[i] + b[i];
    yp[i] = from_f32<T>(gelu_first ? z : adp_gelu(z));
  }
}

// x == 256 fast paths of the per-row modes (0: GELU(LN(a)), 2: LN(GELU(a))): one wave per row, each lane owns 4
// consecutive elements loaded once with one 8- or 16-byte access.
template <typename TA, typename T>
__global__ __launch_bounds__(256) void adapter_row256_kernel(const TA* __restrict__ a, T* __restrict__ y,
                                                             const float* __restrict__ w, const float* __restrict__ b,
                                                             int64_t rows, float eps, int gelu_first) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[4], ww[4], bb[4], o[4];
  Vec<TA, 4>::load(a + row * 256 + lane * 4, v);
  Vec<float, 4>::load(w + lane * 4, ww);
  Vec<float, 4>::load(b + lane * 4, bb);
  if (gelu_first) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = adp_gelu(v[e]);
  }
  const auto [mean, rstd] = adp_row256_stats(v, eps);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float z = (v[e] - mean) * rstd * ww[e] + bb[e];
    o[e] = gelu_first ? z : adp_gelu(z);
  }
  Vec<T, 4>::store(y + row * 256 + lane * 4, o);
}

// backward group pass for the same modes and width: da and the row's (mean, rstd)
template <typename TA, typename T>
__global__ __launch_bounds__(256) void adapter_bwd_row256_kernel(const TA* __restrict__ a, const T* __restrict__ dy,
                                                                 T* __restrict__ da, const float* __restrict__ w,
                                                                 const float* __restrict__ b, float* __restrict__ stats,
                                                                 int64_t rows, float eps, int gelu_first) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float av[4], v[4], dd[4], ww[4], bb[4], g[4], o[4];
  Vec<TA, 4>::load(a + row * 256 + lane * 4, av);
  Vec<T, 4>::load(dy + row * 256 + lane * 4, dd);
  Vec<float, 4>::load(w + lane * 4, ww);
  Vec<float, 4>::load(b + lane * 4, bb);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = gelu_first ? adp_gelu(av[e]) : av[e];
  const auto [mean, rstd] = adp_row256_stats(v, eps);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float nh = (v[e] - mean) * rstd;
    v[e] = nh;
    g[e] = adp_dz(dd[e], nh, ww[e], bb[e], gelu_first) * ww[e];
    s1 += g[e];
    s2 += g[e] * nh;
  }
  const float m1 = wave_sum(s1) * (1.0f / 256.0f), m2 = wave_sum(s2) * (1.0f / 256.0f);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float du = rstd * (g[e] - m1 - v[e] * m2);
    o[e] = gelu_first ? du * adp_gelu_grad(av[e]) : du;
  }
  Vec<T, 4>::store(da + row * 256 + lane * 4, o);
  if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}

// ---- backward, pass 1: one workgroup per normalisation group (frame slab for "nln", row for "ln") -------
// da = rstd * (g - mean(g) - nhat * mean(g * nhat)),  g = dy * gelu'(nhat*w + b) * w;  saves (mean, rstd)
template <typename TA, typename T>
__global__ __launch_bounds__(1024) void adapter_bwd_group_kernel(const TA* __restrict__ a, const T* __restrict__ dy,
                                                                 T* __restrict__ da, const float* __restrict__ w,
                                                                 const float* __restrict__ b, float* __restrict__ stats,
                                                                 int group, int affine_period, float eps, int gelu_first) {
  __shared__ float sc[16];
  const int tid = threadIdx.x;
  const TA* ap = a + (int64_t)blockIdx.x * group;
  const T* dp = dy + (int64_t)blockIdx.x * group;
  T* op = da + (int64_t)blockIdx.x * group;
  const auto sum = [&](float v) { return block_sum(v, sc); };
  // gelu_first: the normalised quantity is u = GELU(a); dL/du = LN backward of dy*w, dL/da = dL/du * GELU'(a)
  const auto [mean, rstd] = adp_strided_stats(ap, gelu_first, tid, blockDim.x, group, eps, sum);
  float s1 = 0.f, s2 = 0.f;
  for (int i = tid; i < group; i += blockDim.x) {
    const int e = i % affine_period;
    const float nh = (adp_in(ap, i, gelu_first) - mean) * rstd;
    const float g = adp_dz(ld(dp + i), nh, w[e], b[e], gelu_first) * w[e];
    s1 += g;
    s2 += g * nh;
  }
  const float m1 = sum(s1) / (float)group, m2 = sum(s2) / (float)group;
  for (int i = tid; i < group; i += blockDim.x) {
    const int e = i % affine_period;
    const float nh = (adp_in(ap, i, gelu_first) - mean) * rstd;
    const float g = adp_dz(ld(dp + i), nh, w[e], b[e], gelu_first) * w[e];
    const float du = rstd * (g - m1 - nh * m2);
    op[i] = from_f32<T>(gelu_first ? du * adp_gelu_grad(ld(ap + i)) : du);
  }
  if (tid == 0) { stats[2 * blockIdx.x] = mean; stats[2 * blockIdx.x + 1] = rstd; }
}

// Register-resident form of the group pass for the joint ("nln") mode: `a` is read once with 16-byte
// loads and kept normalised in registers; dy / weight / bias are streamed twice (second time from L2).
template <typename TA, typename T, int NCH>
__global__ __launch_bounds__(1024) void adapter_bwd_group_reg_kernel(const TA* __restrict__ a, const T* __restrict__ dy,
                                                                     T* __restrict__ da, const float* __restrict__ w,
                                                                     const float* __restrict__ b, float* __restrict__ stats,
                                                                     int group, float eps) {
  __shared__ float sc[16];
  const int tid = threadIdx.x, nchunk = group >> 3;
  const T* dp = dy + (int64_t)blockIdx.x * group;
  T* op = da + (int64_t)blockIdx.x * group;
  float v[NCH][8];
  const auto [mean, rstd] = adp_slab_stats<TA, NCH>(a + (int64_t)blockIdx.x * group, group, eps, v, sc);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = tid + c * 1024;
    if (ch < nchunk) {
      float dd[8], ww[8], bb[8];
      Vec<T, 8>::load(dp + (int64_t)ch * 8, dd);
      Vec<float, 8>::load(w + (int64_t)ch * 8, ww);
      Vec<float, 8>::load(b + (int64_t)ch * 8, bb);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float nh = (v[c][e] - mean) * rstd;
        v[c][e] = nh;  // keep the normalised value
        const float g = adp_dz(dd[e], nh, ww[e], bb[e], 0) * ww[e];
        s1 += g;
        s2 += g * nh;
      }
    }
  }
  const float m1 = block_sum<16>(s1, sc) / (float)group, m2 = block_sum<16>(s2, sc) / (float)group;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = tid + c * 1024;
    if (ch < nchunk) {
      float dd[8], ww[8], bb[8], o[8];
      Vec<T, 8>::load(dp + (int64_t)ch * 8, dd);
      Vec<float, 8>::load(w + (int64_t)ch * 8, ww);
      Vec<float, 8>::load(b + (int64_t)ch * 8, bb);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float nh = v[c][e];
        const float g = adp_dz(dd[e], nh, ww[e], bb[e], 0) * ww[e];
        o[e] = rstd * (g - m1 - nh * m2);
      }
      Vec<T, 8>::store(op + (int64_t)ch * 8, o);
    }
  }
  if (tid == 0) { stats[2 * blockIdx.x] = mean; stats[2 * blockIdx.x + 1] = rstd; }
}

// ---- backward, pass 2: affine gradients.  Thread per affine element e, block-row per chunk of groups;
// partial sums go to slab blockIdx.y and are added in fixed order by adapter_bwd_affine_reduce_kernel.
template <typename TA, typename T>
__global__ __launch_bounds__(256) void adapter_bwd_affine_kernel(const TA* __restrict__ a, const T* __restrict__ dy,
                                                                 const float* __restrict__ w, const float* __restrict__ b,
                                                                 const float* __restrict__ stats, float* __restrict__ part,
                                                                 int64_t groups, int group, int affine, int groups_per_slab,
                                                                 int gelu_first) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= affine) return;
  const int reps = group / affine;  // rows of an affine period inside one group (1 for nln, 1 for ln)
  const int64_t g0 = (int64_t)blockIdx.y * groups_per_slab;
  const int64_t g1 = g0 + groups_per_slab < groups ? g0 + groups_per_slab : groups;
  const float we = w[e], be = b[e];
  float dw = 0.f, db = 0.f;
  for (int64_t gi = g0; gi < g1; ++gi) {
    const float mean = stats[2 * gi], rstd = stats[2 * gi + 1];
    for (int r = 0; r < reps; ++r) {
      const int64_t idx = gi * group + (int64_t)r * affine + e;
      const float nh = (adp_in(a, idx, gelu_first) - mean) * rstd;
      const float dz = adp_dz(ld(dy + idx), nh, we, be, gelu_first);
      dw = fmaf(dz, nh, dw);
      db += dz;
    }
  }
  part[((int64_t)blockIdx.y * 2) * affine + e] = dw;
  part[((int64_t)blockIdx.y * 2 + 1) * affine + e] = db;
}

__global__ void adapter_bwd_affine_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                 int affine, int slabs) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= affine) return;
  float s0 = 0.f, s1 = 0.f;
  for (int z = 0; z < slabs; ++z) { s0 += part[((int64_t)z * 2) * affine + e]; s1 += part[((int64_t)z * 2 + 1) * affine + e]; }
  dw[e] = s0;
  db[e] = s1;
}

// ---- host: one call description, one check, one plan, one launch per direction ------------------------------------
struct AdpCall {
  const void* a = nullptr;
  int a_dtype = DFD_F32;
  void* out = nullptr;       // forward: y; backward: da
  const void* dy = nullptr;  // backward
  int dtype = DFD_F32;       // of y, or of dy and da
  const float *weight = nullptr, *bias = nullptr;
  float *dweight = nullptr, *dbias = nullptr;  // backward
  void* workspace = nullptr;                   // backward: the groups' (mean, rstd), then the affine partial slabs
  int frames = 0, patches = 0, x = 0;
  int mode = 0;  // 0: GELU(LN(a)) per row; 1: joint over a frame's (patches, x) slab; 2: LN(GELU(a)) per row
  float eps = 0.f;
  bool no_pointers = false;  // the plan hook's call: nothing to check or read but `misaligned`
  bool misaligned = false;   // no_pointers: what the hook was told
};

struct AdpPlan {
  int path = 0;                   // DFD_ADP_* of the forward kernel or the backward's group pass; 0: nothing to launch
  int64_t grid = 0;               // of that kernel, as computed: adp_check refuses what does not fit a grid dimension
  unsigned block = 0;
  int64_t groups = 0;             // normalisation groups: frames (joint) or rows
  int64_t group = 0;              // elements of one, which is also the affine's extent
  int slabs = 0, groups_per_slab = 0;  // backward: the affine pass's partial slabs
};

constexpr int64_t kAdpRegLimit = 1024 * 8 * 7;  // register-resident slab: 7 chunks x 1024 threads x 8 elements

int affine_slabs(int64_t groups, int64_t affine) {
  // enough (element, chunk) threads to cover the chip; at most 512 slabs
  int64_t want = (262144 + affine - 1) / affine;
  if (want > groups) want = groups;
  if (want > 512) want = 512;
  if (want < 1) want = 1;
  return (int)want;
}

// The vector kernels' 16-byte accesses: a, the output, dy (backward), weight and bias.
bool adp_misaligned(const AdpCall& c) {
  if (c.no_pointers) return c.misaligned;
  return !(dfd_aligned16(c.a) && dfd_aligned16(c.out) && dfd_aligned16(c.dy) && dfd_aligned16(c.weight) && dfd_aligned16(c.bias));
}

// Which kernel serves a call and with which launch; the table is in include/dfdclip_hooks.h.  Wants positive patches
// and x; everything is computed in 64 bits, so it may run before adp_check has bounded the extents.
AdpPlan adp_plan(const AdpCall& c, bool backward) {
  AdpPlan p;
  const bool joint = c.mode == 1, vec = !adp_misaligned(c);
  p.groups = joint ? c.frames : (int64_t)c.frames * c.patches;
  p.group = joint ? (int64_t)c.patches * c.x : c.x;
  if (p.groups <= 0) return p;
  if (joint) {
    p.path = vec && p.group % 8 == 0 && p.group <= kAdpRegLimit ? DFD_ADP_JOINT_REG : DFD_ADP_JOINT;
    p.grid = p.groups, p.block = 1024;
  } else if (vec && c.x == 256) {
    p.path = DFD_ADP_ROW256, p.grid = (p.groups + 3) / 4, p.block = 256;
  } else {  // one wave per row: four to a workgroup forward, a workgroup of its own backward
    p.path = DFD_ADP_ROW, p.grid = backward ? p.groups : (p.groups + 3) / 4, p.block = backward ? 64 : 256;
  }
  if (backward) {
    p.slabs = affine_slabs(p.groups, p.group);
    p.groups_per_slab = (int)((p.groups + p.slabs - 1) / p.slabs);
  }
  return p;
}

// Every rule of dfd_adapter_norm_gelu and dfd_adapter_norm_gelu_bwd, under the entry point's name.  Forward takes
// frames == 0 (nothing is launched) and y == a where the two have one dtype; backward needs frames > 0, its workspace,
// and a da that is neither dy nor a.
int adp_check(const char* fn, const AdpCall& c, bool backward) {
  DFD_REQUIRE(c.no_pointers || (c.a && c.out && c.weight && c.bias && (!backward || (c.dy && c.dweight && c.dbias && c.workspace))),
              "%s: null pointer", fn);
  DFD_REQUIRE(c.frames >= (backward ? 1 : 0) && c.patches > 0 && c.x > 0, "%s: bad shape", fn);
  DFD_REQUIRE(c.no_pointers || !backward || (c.out != c.dy && c.out != c.a),
              "%s: da must not alias dy or a (both are re-read by the affine pass)", fn);
  DFD_REQUIRE(ok_dtype(c.dtype), "%s: dtype=%d", fn, c.dtype);
  DFD_REQUIRE(c.a_dtype == c.dtype || c.a_dtype == DFD_F32, "%s: a_dtype=%d must be dtype or f32", fn, c.a_dtype);
  DFD_REQUIRE(c.no_pointers || backward || c.a_dtype == c.dtype || c.a != c.out, "%s: in place needs one dtype", fn);
  DFD_REQUIRE(c.mode >= 0 && c.mode <= 2, "%s: mode=%d", fn, c.mode);
  DFD_REQUIRE((int64_t)c.patches * c.x < (1ll << 31), "%s: patches * x = %lld must be below 2^31", fn, (long long)c.patches * c.x);
  DFD_REQUIRE(adp_plan(c, backward).grid <= 0x7fffffff, "%s: frames=%d patches=%d: the groups do not fit a grid of 2^31 - 1", fn,
              c.frames, c.patches);
  return DFD_OK;
}

thread_local int g_adp_last_path = 0;

int adp_launch_fwd(const char* fn, const AdpCall& c, const AdpPlan& p, hipStream_t st) {
  const dim3 grid((unsigned)p.grid), block(p.block);
  const int slab = (int)p.group, gelu_first = c.mode == 2;
  with_types<false>(c.a_dtype, c.dtype, [&](auto ta, auto t) {
    using TA = typename decltype(ta)::type;
    using T = typename decltype(t)::type;
    const TA* a = static_cast<const TA*>(c.a);
    T* y = static_cast<T*>(c.out);
    if (p.path == DFD_ADP_JOINT_REG)
      hipLaunchKernelGGL((adapter_nln_reg_kernel<TA, T, 7>), grid, block, 0, st, a, y, c.weight, c.bias, slab, c.eps);
    else if (p.path == DFD_ADP_JOINT)
      hipLaunchKernelGGL((adapter_nln_kernel<TA, T>), grid, block, 0, st, a, y, c.weight, c.bias, slab, c.eps);
    else if (p.path == DFD_ADP_ROW256)
      hipLaunchKernelGGL((adapter_row256_kernel<TA, T>), grid, block, 0, st, a, y, c.weight, c.bias, p.groups, c.eps, gelu_first);
    else
      hipLaunchKernelGGL((adapter_ln_kernel<TA, T>), grid, block, 0, st, a, y, c.weight, c.bias, p.groups, c.x, c.eps, gelu_first);
  });
  DFD_CHECK_LAUNCH(fn);
  return DFD_OK;
}

// group pass, affine partials, affine reduction: three launches under one launch check
int adp_launch_bwd(const char* fn, const AdpCall& c, const AdpPlan& p, hipStream_t st) {
  const dim3 grid((unsigned)p.grid), block(p.block);
  const int group = (int)p.group, affine = group, gelu_first = c.mode == 2;
  float* stats = static_cast<float*>(c.workspace);
  float* part = stats + p.groups * 2;
  with_types<false>(c.a_dtype, c.dtype, [&](auto ta, auto t) {
    using TA = typename decltype(ta)::type;
    using T = typename decltype(t)::type;
    const TA* a = static_cast<const TA*>(c.a);
    const T* dy = static_cast<const T*>(c.dy);
    T* da = static_cast<T*>(c.out);
    if (p.path == DFD_ADP_ROW256)
      hipLaunchKernelGGL((adapter_bwd_row256_kernel<TA, T>), grid, block, 0, st, a, dy, da, c.weight, c.bias, stats, p.groups, c.eps,
                         gelu_first);
    else if (p.path == DFD_ADP_JOINT_REG)
      hipLaunchKernelGGL((adapter_bwd_group_reg_kernel<TA, T, 7>), grid, block, 0, st, a, dy, da, c.weight, c.bias, stats, group, c.eps);
    else
      hipLaunchKernelGGL((adapter_bwd_group_kernel<TA, T>), grid, block, 0, st, a, dy, da, c.weight, c.bias, stats, group, affine,
                         c.eps, gelu_first);
    hipLaunchKernelGGL((adapter_bwd_affine_kernel<TA, T>), dim3((affine + 255) / 256, p.slabs), dim3(256), 0, st, a, dy, c.weight,
                       c.bias, stats, part, p.groups, group, affine, p.groups_per_slab, gelu_first);
  });
  hipLaunchKernelGGL(adapter_bwd_affine_reduce_kernel, dim3((affine + 255) / 256), dim3(256), 0, st, part, c.dweight, c.dbias, affine,
                     p.slabs);
  DFD_CHECK_LAUNCH(fn);
  return DFD_OK;
}

int adp_run(const char* fn, const AdpCall& c, bool backward, void* stream) {
  if (int rc = adp_check(fn, c, backward)) return rc;
  const AdpPlan p = adp_plan(c, backward);
  if (p.path == 0) return DFD_OK;  // forward with frames == 0
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = backward ? adp_launch_bwd(fn, c, p, st) : adp_launch_fwd(fn, c, p, st)) return rc;
  g_adp_last_path = p.path;
  return DFD_OK;
}

}  // namespace

extern "C" size_t dfd_adapter_norm_gelu_bwd_workspace(int frames, int patches, int x, int joint) {
  if (frames <= 0 || patches <= 0 || x <= 0 || (int64_t)patches * x >= (1ll << 31)) return 0;
  AdpCall c;
  c.frames = frames, c.patches = patches, c.x = x, c.mode = joint == 1, c.no_pointers = true;
  const AdpPlan p = adp_plan(c, true);
  return (size_t)p.groups * 2 * sizeof(float) + (size_t)p.slabs * 2 * (size_t)p.group * sizeof(float);
}

extern "C" int dfd_adapter_norm_gelu_bwd(const void* a, int a_dtype, const void* dy, void* da, int dtype, const float* weight,
                                         const float* bias, float* dweight, float* dbias, void* workspace, int frames,
                                         int patches, int x, int joint, float eps, void* stream) {
  AdpCall c;
  c.a = a, c.a_dtype = a_dtype, c.dy = dy, c.out = da, c.dtype = dtype, c.weight = weight, c.bias = bias;
  c.dweight = dweight, c.dbias = dbias, c.workspace = workspace;
  c.frames = frames, c.patches = patches, c.x = x, c.mode = joint, c.eps = eps;
  return adp_run("dfd_adapter_norm_gelu_bwd", c, true, stream);
}

extern "C" int dfd_adapter_norm_gelu(const void* a, int a_dtype, void* y, int dtype, const float* weight, const float* bias, int frames,
                                     int patches, int x, int joint, float eps, void* stream) {
  AdpCall c;
  c.a = a, c.a_dtype = a_dtype, c.out = y, c.dtype = dtype, c.weight = weight, c.bias = bias;
  c.frames = frames, c.patches = patches, c.x = x, c.mode = joint, c.eps = eps;
  return adp_run("dfd_adapter_norm_gelu", c, false, stream);
}

extern "C" int dfd_adapter_norm_gelu_last_path(void) { return g_adp_last_path; }

extern "C" int dfd_adapter_norm_gelu_plan(int frames, int patches, int x, int joint, int a_dtype, int dtype, int misaligned, int backward,
                                          dfd_adapter_plan_t* out) {
  const char* fn = backward ? "dfd_adapter_norm_gelu_bwd" : "dfd_adapter_norm_gelu";
  AdpCall c;
  c.a_dtype = a_dtype, c.dtype = dtype, c.frames = frames, c.patches = patches, c.x = x, c.mode = joint;
  c.no_pointers = true, c.misaligned = misaligned != 0;
  if (adp_check(fn, c, backward != 0) != DFD_OK) return -1;
  const AdpPlan p = adp_plan(c, backward != 0);
  if (out) *out = dfd_adapter_plan_t{p.path, (uint32_t)p.grid, p.block, p.slabs, p.groups_per_slab};
  return p.path;
}
