// Fused optimizer step over a list of f32 parameters: SGD with momentum 0.95 or AdamW, with the config's weight decay, over
// the trainable parameters (reference src/models.py:740-754, stepped once per batch by src/trainer.py:157-177), and AdamW
// over the adapter (src/models.py:1053-1057).  One launch per step where torch's multi-tensor paths take several (SGD ten;
// AdamW: tools/bench_adamw.py counts them), and for the decoder's Linear weights the launch also rewrites the transposed
// f32 copy the row-streaming linear kernels read (dfd_linear_rows_t): the 20 transposes a training step otherwise needs
// after every update disappear.  The EMA teacher's update (dfd_ema_step, include/dfdclip_ema.h) walks the same table.
//
// SGD's arithmetic, per element, in torch's order (torch/optim/sgd.py, foreach path; AdamW's stands at its kernel):
//     g   = grad + wd * p                (one fused multiply-add)
//     buf = first step ? g : momentum * buf + g      (product rounded, then the sum)
//     p   = p - lr * buf                 (one fused multiply-add)
// Workgroups are dealt to parameters through a table in device memory (binary search on the first block of each entry):
// an entry is either a flat run of 1,024 elements per block or, for a mirrored [rows, cols] weight, 32 x 32 tiles whose
// transposed image goes through LDS so that both the parameter and its mirror are written in whole row segments.
#include <cmath>
#include <cstddef>

#include "stream_policy.hpp"
#include "../../include/dfdclip_ema.h"

namespace {

struct SgdEntry {      // mirrors dfd_sgd_param of the C ABI
  float* p;
  const float* g;
  float* buf;
  float* mirror;       // [cols, rows] transposed copy, or NULL
  int64_t numel;
  int32_t rows, cols;  // only read when mirror != NULL
  int64_t first_block;
};

// The traversal both optimizers share: find this workgroup's entry, then hand `update(entry index, entry, element)`
// (which returns the new parameter value) every element of its block or tile.
// NT (DFD_STREAM_OPTIMIZER): every byte here is touched once per step, and the mirror's next reader is a step away.
template <bool NT, class Update>
__device__ __forceinline__ void step_entries(const SgdEntry* __restrict__ table, int n, float (*tile)[33], Update update) {
  const int64_t b = blockIdx.x;
  int lo = 0, hi = n - 1;  // last entry whose first_block <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_block <= b) lo = mid;
    else hi = mid - 1;
  }
  const SgdEntry e = table[lo];
  const int64_t lb = b - e.first_block;
  if (e.mirror == nullptr) {
    const int64_t i0 = lb * 1024 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i = i0 + k * 256;
      if (i < e.numel) update(lo, e, i);
    }
    return;
  }
  const int tiles_c = (e.cols + 31) / 32;
  const int tr = (int)(lb / tiles_c), tc = (int)(lb - (int64_t)tr * tiles_c);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8 threads, four rows each
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = tr * 32 + ty + 8 * k, c = tc * 32 + tx;
    if (r < e.rows && c < e.cols) tile[ty + 8 * k][tx] = update(lo, e, (int64_t)r * e.cols + c);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = tc * 32 + ty + 8 * k, r = tr * 32 + tx;  // mirror row = parameter column
    if (r < e.rows && c < e.cols) stream_store4<NT>(e.mirror + (int64_t)c * e.rows + r, tile[tx][ty + 8 * k]);
  }
}

template <bool NT>
__global__ __launch_bounds__(256) void sgd_step_kernel(const SgdEntry* __restrict__ table, int n, float lr, float momentum, float wd, int first) {
  __shared__ float tile[32][33];
  step_entries<NT>(table, n, tile, [&](int, const SgdEntry& e, int64_t i) {
    const float p = stream_load4<NT>(e.p + i);
    const float g = __builtin_fmaf(wd, p, stream_load4<NT>(e.g + i));
    float m = g;
    if (!first) m = momentum * stream_load4<NT>(e.buf + i) + g;
    stream_store4<NT>(e.buf + i, m);
    const float np = __builtin_fmaf(-lr, m, p);
    stream_store4<NT>(e.p + i, np);
    return np;
  });
}

// AdamW in the order of torch 2.10's _multi_tensor_adam (non-capturable, decoupled weight decay), one rounding per foreach
// op of that path.  Every scalar is formed in double on the host and cast to float once, as torch's kernels cast theirs;
// the betas and eps arrive as the doubles torch holds, lr and wd as the entry point's floats, so `decay` and `step_size`
// are formed from float-rounded inputs and can be 1 ulp from torch's (a relative 6e-8 of a step's change of p):
//     p   = p * decay                          (decay = 1 - lr wd; skipped when wd == 0)
//     m   = lerp(m, g, w1)                     (w1 = 1 - beta1; torch's lerp: m + w1 (g - m) below 0.5, g - (g - m)(1 - w1) from there)
//     v   = v * beta2;  v = v + w2 (g g)       (w2 = 1 - beta2)
//     den = sqrt(v) / bc2_sqrt + eps           (bc2_sqrt = sqrt(1 - beta2^step))
//     p   = p + step_size (m / den)            (step_size = -lr / (1 - beta1^step))
// `buf` of an entry is exp_avg; exp_avg_sq of entry i is vs[i].
struct AdamwArgs {
  float decay, w1, beta2, w2, bc2_sqrt, eps, step_size;
  int decay_on;
};

template <bool NT>
__global__ __launch_bounds__(256) void adamw_step_kernel(const SgdEntry* __restrict__ table, int n, float* const* __restrict__ vs, AdamwArgs a) {
  __shared__ float tile[32][33];
  step_entries<NT>(table, n, tile, [&](int idx, const SgdEntry& e, int64_t i) {
    float* __restrict__ vv = vs[idx];
    float p = stream_load4<NT>(e.p + i);
    const float g = stream_load4<NT>(e.g + i);
    float m = stream_load4<NT>(e.buf + i), v = stream_load4<NT>(vv + i);
    if (a.decay_on) p *= a.decay;
    const float d = g - m;
    m = a.w1 < 0.5f ? __builtin_fmaf(a.w1, d, m) : __builtin_fmaf(-d, 1.0f - a.w1, g);
    v *= a.beta2;
    v = __builtin_fmaf(a.w2, g * g, v);
    stream_store4<NT>(e.buf + i, m);
    stream_store4<NT>(vv + i, v);
    const float den = __builtin_sqrtf(v) / a.bc2_sqrt + a.eps;
    p = __builtin_fmaf(a.step_size, m / den, p);
    stream_store4<NT>(e.p + i, p);
    return p;
  });
}

// The teacher's exponential moving average (reference src/trainer.py:179-185: p_t <- (1 - r) p_t + r p) over the same table:
// `p` the teacher's parameter, `g` the student's, `buf` unused.  torch evaluates the expression on f32 tensors as two
// products, each rounded, and one sum: contracted into a fused multiply-add the result differs in the last bit, so
// contraction is switched off for exactly this expression.
__device__ __forceinline__ float ema_blend(float keep, float t, float take, float s) {
#pragma clang fp contract(off)
  const float a = keep * t;
  const float b = take * s;
  return a + b;
}

template <bool NT>
__global__ __launch_bounds__(256) void ema_step_kernel(const SgdEntry* __restrict__ table, int n, float keep, float take) {
  __shared__ float tile[32][33];
  step_entries<NT>(table, n, tile, [&](int, const SgdEntry& e, int64_t i) {
    const float nt = ema_blend(keep, stream_load4<NT>(e.p + i), take, stream_load4<NT>(e.g + i));
    stream_store4<NT>(e.p + i, nt);
    return nt;
  });
}

}  // namespace

static_assert(sizeof(SgdEntry) == sizeof(dfd_sgd_param), "dfd_sgd_param layout");
static_assert(sizeof(dfd_optim_extra) == 48 && offsetof(dfd_optim_extra, beta1) == 8 && offsetof(dfd_optim_extra, step) == 32 &&
                  offsetof(dfd_optim_extra, exp_avg_sq) == 40,
              "dfd_optim_extra layout");

extern "C" int64_t dfd_sgd_blocks(int64_t numel, int rows, int cols, int mirrored) {
  if (mirrored) return (int64_t)((rows + 31) / 32) * ((cols + 31) / 32);
  return (numel + 1023) / 1024;
}

extern "C" int dfd_sgd_step(const dfd_sgd_param* table_dev, int n, int64_t total_blocks, float lr, float momentum, float weight_decay,
                            int first_step, void* stream, const dfd_optim_extra* extra) {
  DFD_REQUIRE(extra == nullptr || extra->kind == DFD_OPTIM_SGD || extra->kind == DFD_OPTIM_ADAMW, "dfd_sgd_step: unknown kind %d",
              extra->kind);
  DFD_REQUIRE(table_dev != nullptr && n > 0, "dfd_sgd_step: empty table");
  DFD_REQUIRE(total_blocks > 0 && total_blocks < ((int64_t)1 << 31), "dfd_sgd_step: total_blocks = %lld", (long long)total_blocks);
  const auto* table = reinterpret_cast<const SgdEntry*>(table_dev);
  const bool nt = dfd_stream_on(DFD_STREAM_OPTIMIZER);
  if (extra == nullptr || extra->kind == DFD_OPTIM_SGD) {
    hipLaunchKernelGGL(nt ? sgd_step_kernel<true> : sgd_step_kernel<false>, dim3((unsigned)total_blocks), dim3(256), 0, static_cast<hipStream_t>(stream), table, n, lr,
                       momentum, weight_decay, first_step);
    DFD_CHECK_LAUNCH("dfd_sgd_step");
    return DFD_OK;
  }
  const double b1 = extra->beta1, b2 = extra->beta2;
  DFD_REQUIRE(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, "dfd_sgd_step: AdamW betas (%g, %g) outside [0, 1)", b1, b2);
  DFD_REQUIRE(extra->eps > 0.0, "dfd_sgd_step: AdamW eps = %g", extra->eps);
  DFD_REQUIRE(extra->step >= 1, "dfd_sgd_step: AdamW step count %lld (the count after this step, >= 1)", (long long)extra->step);
  DFD_REQUIRE(extra->exp_avg_sq != nullptr, "dfd_sgd_step: AdamW without its second moments (null pointer)");
  // torch forms these in Python floats (doubles) and hands each foreach kernel a scalar that is cast to float there; lr and
  // weight_decay are already floats here (see the kernel's comment)
  const double t = (double)extra->step, lrd = lr, wdd = weight_decay;
  AdamwArgs a;
  a.decay = (float)(1.0 - lrd * wdd);
  a.decay_on = weight_decay != 0.0f;
  a.w1 = (float)(1.0 - b1);
  a.beta2 = (float)b2;
  a.w2 = (float)(1.0 - b2);
  a.bc2_sqrt = (float)std::pow(1.0 - std::pow(b2, t), 0.5);
  a.eps = (float)extra->eps;
  a.step_size = (float)((lrd / (1.0 - std::pow(b1, t))) * -1.0);
  hipLaunchKernelGGL(nt ? adamw_step_kernel<true> : adamw_step_kernel<false>, dim3((unsigned)total_blocks), dim3(256), 0, static_cast<hipStream_t>(stream), table, n,
                     extra->exp_avg_sq, a);
  DFD_CHECK_LAUNCH("dfd_sgd_step");
  return DFD_OK;
}

extern "C" int dfd_ema_step(const dfd_sgd_param* table_dev, int n, int64_t total_blocks, float keep, float take, void* stream) {
  DFD_REQUIRE(table_dev != nullptr && n > 0, "dfd_ema_step: empty table (table=%p, n=%d)", (const void*)table_dev, n);
  DFD_REQUIRE(total_blocks > 0 && total_blocks < ((int64_t)1 << 31), "dfd_ema_step: total_blocks = %lld outside [1, 2^31)",
              (long long)total_blocks);
  DFD_REQUIRE(std::isfinite(keep) && std::isfinite(take), "dfd_ema_step: non-finite factor (keep=%g, take=%g)", (double)keep, (double)take);
  const auto* table = reinterpret_cast<const SgdEntry*>(table_dev);
  const bool nt = dfd_stream_on(DFD_STREAM_OPTIMIZER);
  hipLaunchKernelGGL(nt ? ema_step_kernel<true> : ema_step_kernel<false>, dim3((unsigned)total_blocks), dim3(256), 0, static_cast<hipStream_t>(stream), table, n,
                     keep, take);
  DFD_CHECK_LAUNCH("dfd_ema_step");
  return DFD_OK;
}
