// C = epilogue(A[M,K] · W[N,K]ᵀ) on the gfx950 matrix cores — the encoder's four GEMM shapes
// (QKV, out_proj, c_fc, c_proj; reference clip/model.py:186, :197, :208-212) plus the patch
// conv as a GEMM (clip/model.py:277).
//
// gemm128: general-shape kernel.  128x128 output tile per 256-thread workgroup (4 waves as
//   2x2, each wave a 64x64 patch = 2x2 MFMA 32x32 tiles), K consumed 64 BYTES per row per step
//   (32 bf16 / 16 f32), LDS rows padded to 80 B, double-buffered LDS with the next tile's
//   global loads in flight across the MFMA block.  bf16 operands use v_mfma_f32_32x32x16_bf16;
//   f32 operands use v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain — the 1e-3 parity path).
//   Any M, N; K % 32 == 0.  Out-of-range rows load zeros and are not stored.
//
// Both A and W are K-contiguous, so both MFMA operands are plain 16-byte row reads: lane
// (r = lane&31, h = lane>>5) holds A[row r][k-slice h] and W[row r][k-slice h].
#include "gemm_plan.hpp"
#include "gelu.hpp"

namespace {

constexpr int BM = 128, BN = 128;
constexpr int ROW_BYTES = 64;   // K bytes per row per step
constexpr int ROW_STRIDE = 80;  // padded LDS row
constexpr int TILE_BYTES = BM * ROW_STRIDE;
constexpr int EPI_SPLITK_SLAB = 100;  // internal: raw f32 accumulators to slab blockIdx.z of C

template <typename CT> __device__ __forceinline__ void store_c(void* C, int64_t off, float v) {
  static_cast<CT*>(C)[off] = from_f32<CT>(v);
}

template <typename CT, int EPI>
__device__ __forceinline__ void epilogue_elem(const GemmArgs& a, int64_t m, int n, float acc) {
  if (m >= a.M || n >= a.N) return;
  if constexpr (EPI == DFD_EPI_BIAS) {
    store_c<CT>(a.C, m * a.ldc + n, acc + (a.bias ? a.bias[n] : 0.f));
  } else if constexpr (EPI == DFD_EPI_BIAS_QUICKGELU) {
    store_c<CT>(a.C, m * a.ldc + n, quick_gelu(acc + (a.bias ? a.bias[n] : 0.f)));
  } else if constexpr (EPI == DFD_EPI_BIAS_GELU) {
    store_c<CT>(a.C, m * a.ldc + n, gelu_erf(acc + (a.bias ? a.bias[n] : 0.f)));
  } else if constexpr (EPI == DFD_EPI_BIAS_RESIDUAL) {
    float* c = static_cast<float*>(a.C) + m * a.ldc + n;
    *c = *c + (acc + (a.bias ? a.bias[n] : 0.f));
  } else if constexpr (EPI == DFD_EPI_PATCH_EMBED) {
    const int P = a.tokens - 1;
    const int64_t frame = m / P;
    const int p = (int)(m - frame * P);
    float* c = static_cast<float*>(a.C);
    c[(frame * a.tokens + 1 + p) * a.ldc + n] = acc + a.pos[(int64_t)(1 + p) * a.N + n];
    if (p == 0) c[(frame * a.tokens) * a.ldc + n] = a.cls[n] + a.pos[n];
  } else if constexpr (EPI == DFD_EPI_RESIDUAL_POS) {
    const int64_t frame = m / (a.tokens - 1);
    const float p = a.pos ? a.pos[(frame % a.frames_per_clip) * a.N + n] : 0.f;
    CT* c = static_cast<CT*>(a.C) + m * a.ldc + n;
    const CT* rsd = a.residual ? static_cast<const CT*>(a.residual) + m * a.ldc + n : c;
    *c = from_f32<CT>(to_f32(*rsd) + dfd_drop_one(a.drop, (uint64_t)m * a.N + n, acc) + p);
  } else if constexpr (EPI == DFD_EPI_QKV_EXPORT) {
    const float v = acc + (a.bias ? a.bias[n] : 0.f);
    store_c<CT>(a.C, m * a.ldc + n, v);
    const int D = a.N / (3 - a.qkv_first);
    const int ne = n + a.qkv_first * D;  // column in the full [q | k | v] numbering
    if (a.k_export != nullptr && ne >= D) {
      const int64_t frame = m / a.tokens;
      const int tok = (int)(m - frame * a.tokens);
      if (tok > 0) {
        const bool is_v = ne >= 2 * D;
        const int cc = ne - (is_v ? 2 * D : D);
        const float e = v + (a.pos ? a.pos[(frame % a.frames_per_clip) * D + cc] : 0.f);
        store_c<CT>(is_v ? a.v_export : a.k_export, (frame * (a.tokens - 1) + tok - 1) * D + cc, e);
      }
    }
  }
}

template <typename T, typename CT, int EPI>
__global__ __launch_bounds__(256) void gemm128_kernel(const GemmArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILE_BYTES];  // A0 A1 B0 B1
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;
  constexpr int KSTEP = ROW_BYTES / (int)sizeof(T);  // elements of K per step
  // split-K (gridDim.z > 1): slice z covers K steps [z*per, (z+1)*per) and writes its own f32 slab of C
  const int nk_all = a.K / KSTEP;
  const int per = (nk_all + (int)gridDim.z - 1) / (int)gridDim.z;
  const int kt0 = (int)blockIdx.z * per;
  const int nk = min(per, nk_all - kt0) > 0 ? min(per, nk_all - kt0) : 0;

  // staging assignment: 512 16-byte chunks per matrix tile, 2 per thread
  const unsigned char* Ab = static_cast<const unsigned char*>(a.A);
  const unsigned char* Wb = static_cast<const unsigned char*>(a.W);
  uint4 ra[2], rb[2];
  int srow[2], scol[2];
  bool va[2], vb[2];
  const unsigned char* pa[2];
  const unsigned char* pb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = tid + 256 * i;
    srow[i] = c >> 2;
    scol[i] = (c & 3) * 16;
    va[i] = (m0 + srow[i]) < a.M;
    vb[i] = (n0 + srow[i]) < a.N;
    pa[i] = Ab + ((m0 + srow[i]) * a.lda) * (int64_t)sizeof(T) + scol[i];
    pb[i] = Wb + ((int64_t)(n0 + srow[i]) * a.ldw) * (int64_t)sizeof(T) + scol[i];
  }
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ra[i] = va[i] ? *reinterpret_cast<const uint4*>(pa[i] + (int64_t)(kt0 + kt) * ROW_BYTES) : uint4{0, 0, 0, 0};
      rb[i] = vb[i] ? *reinterpret_cast<const uint4*>(pb[i] + (int64_t)(kt0 + kt) * ROW_BYTES) : uint4{0, 0, 0, 0};
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<uint4*>(smem + buf * TILE_BYTES + srow[i] * ROW_STRIDE + scol[i]) = ra[i];
      *reinterpret_cast<uint4*>(smem + (2 + buf) * TILE_BYTES + srow[i] * ROW_STRIDE + scol[i]) = rb[i];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  if (nk > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    const unsigned char* As = smem + buf * TILE_BYTES + (wm * 64 + r) * ROW_STRIDE;
    const unsigned char* Bs = smem + (2 + buf) * TILE_BYTES + (wn * 64 + r) * ROW_STRIDE;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[i] = *reinterpret_cast<const bf16x8*>(As + i * 32 * ROW_STRIDE + s * 32 + h * 16);
          fb[i] = *reinterpret_cast<const bf16x8*>(Bs + i * 32 * ROW_STRIDE + s * 32 + h * 16);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    } else {
      // f32: lane half h owns k-slice [8h, 8h+8) of the 16-wide step; MFMA step s pairs k = s and
      // k = 8 + s (any pairing is valid as long as A and W use the same one).
      f32x4 fa[2][2], fb[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          fa[i][q] = *reinterpret_cast<const f32x4*>(As + i * 32 * ROW_STRIDE + h * 32 + q * 16);
          fb[i][q] = *reinterpret_cast<const f32x4*>(Bs + i * 32 * ROW_STRIDE + h * 32 + q * 16);
        }
#pragma unroll
      for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][s >> 2][s & 3], fb[j][s >> 2][s & 3], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tile(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        const int n = n0 + wn * 64 + j * 32 + r;
        if constexpr (EPI == EPI_SPLITK_SLAB) {
          if (m < a.M && n < a.N) static_cast<float*>(a.C)[((int64_t)blockIdx.z * a.M + m) * a.ldc + n] = acc[i][j][e];
        } else {
          epilogue_elem<CT, EPI>(a, m, n, acc[i][j][e]);
        }
      }
}

// (epilogue) -> instantiation; BIAS_RESIDUAL and PATCH_EMBED exist for an f32 C only (gemm_general_refuses, gemm_plan.hpp)
template <typename T, typename CT>
int launch_gemm128(const GemmPlan& p, const GemmArgs& a, hipStream_t st) {
#define EPI_CASE(E) \
  case E:           \
    return gemm_launch<&gemm128_kernel<T, CT, E>>("general", p, st, a);
  switch (p.epilogue) {
    EPI_CASE(DFD_EPI_BIAS)
    EPI_CASE(DFD_EPI_BIAS_QUICKGELU)
    EPI_CASE(DFD_EPI_BIAS_GELU)
    EPI_CASE(DFD_EPI_QKV_EXPORT)
    EPI_CASE(DFD_EPI_RESIDUAL_POS)
    default:
      if constexpr (sizeof(CT) == 4) {
        switch (p.epilogue) {
          EPI_CASE(DFD_EPI_BIAS_RESIDUAL)
          EPI_CASE(DFD_EPI_PATCH_EMBED)
        }
      }
      return DFD_ERR_INVALID_ARG;  // not reached: the plan names no other epilogue
  }
#undef EPI_CASE
}

// ---- C = Aᵀ·B for tall operands (weight gradients): transposes + split-K on the kernel above ----------
template <typename T>
__global__ __launch_bounds__(256) void transpose_pad_kernel(const T* __restrict__ src, int64_t lds_, T* __restrict__ dst, int64_t R,
                                                            int C, int64_t Rp) {
  __shared__ T tile[32][33];
  const int c0 = blockIdx.x * 32;
  const int64_t r0 = (int64_t)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) tile[i][tx] = (r0 + i < R && c0 + tx < C) ? src[(r0 + i) * lds_ + c0 + tx] : from_f32<T>(0.f);
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (c0 + i < C && r0 + tx < Rp) dst[(int64_t)(c0 + i) * Rp + r0 + tx] = tile[tx][i];
}

__global__ void slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out, int64_t n, int splits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int z = 0; z < splits; ++z) s += slabs[(int64_t)z * n + i];
  out[i] = s;
}

void at_b_plan(int64_t R, int Ma, int Nb, int64_t* Rp, int* splits) {
  const int tiles = ((Ma + BM - 1) / BM) * ((Nb + BN - 1) / BN);
  int sp = (1024 + tiles - 1) / tiles;                       // ~4 workgroups per CU in flight
  const int64_t steps = (R + 31) / 32;
  if (sp > steps / 8) sp = (int)(steps / 8 > 0 ? steps / 8 : 1);  // at least 8 K steps per slice
  if (sp > 512) sp = 512;
  *splits = sp;
  *Rp = (R + 31) / 32 * 32;
}

template <typename T>
int launch_at_b(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t R, int Ma, int Nb, void* workspace,
                hipStream_t st) {
  int64_t Rp;
  int splits;
  at_b_plan(R, Ma, Nb, &Rp, &splits);
  T* At = static_cast<T*>(workspace);
  T* Bt = At + (int64_t)Ma * Rp;
  size_t off = (size_t)(Ma + Nb) * Rp * sizeof(T);
  off = (off + 255) / 256 * 256;
  float* slabs = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + off);
  const dim3 tb(256);
  hipLaunchKernelGGL((transpose_pad_kernel<T>), dim3((Ma + 31) / 32, (unsigned)(Rp / 32)), tb, 0, st, static_cast<const T*>(A), lda, At, R, Ma, Rp);
  hipLaunchKernelGGL((transpose_pad_kernel<T>), dim3((Nb + 31) / 32, (unsigned)(Rp / 32)), tb, 0, st, static_cast<const T*>(B), ldb, Bt, R, Nb, Rp);
  GemmArgs a{};
  a.A = At; a.W = Bt; a.C = slabs; a.lda = Rp; a.ldw = Rp; a.ldc = Nb; a.M = Ma; a.N = Nb; a.K = (int)Rp;
  const dim3 grid((Nb + BN - 1) / BN, (Ma + BM - 1) / BM, splits);
  hipLaunchKernelGGL((gemm128_kernel<T, float, EPI_SPLITK_SLAB>), grid, tb, 0, st, a);
  const int64_t n = (int64_t)Ma * Nb;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((n + 255) / 256)), tb, 0, st, slabs, C, n, splits);
  DFD_CHECK_LAUNCH("dfd_gemm_at_b");
  return DFD_OK;
}

}  // namespace

// copy of dfd_gemm_extra into the kernels' argument block, and the two checks that need its pointers or its dropout
static int fill_extra(GemmArgs& a, int epilogue, const dfd_gemm_extra* extra) {
  if (!extra) return DFD_OK;
  a.pos = extra->pos; a.cls = extra->cls; a.k_export = extra->k_export; a.v_export = extra->v_export;
  a.residual = epilogue == DFD_EPI_RESIDUAL_POS ? extra->residual : nullptr;
  a.tokens = extra->tokens; a.frames_per_clip = extra->frames_per_clip;
  a.qkv_first = epilogue == DFD_EPI_QKV_EXPORT ? extra->qkv_first : 0;
  a.stream_out = (extra->flags & DFD_GEMM_STREAM_OUT) ? 1 : 0;
  a.spare_cus = (int)((extra->flags >> DFD_GEMM_SPARE_CUS_SHIFT) & 0xff);
  a.spare_if_free = (extra->flags & DFD_GEMM_SPARE_IF_FREE) ? 1 : 0;
  a.tile_rows = 32 * (int)((extra->flags >> DFD_GEMM_TILE_BLOCKS_SHIFT) & 0xf);
  a.c_blocked = (extra->flags & DFD_GEMM_C_BLOCKED) ? 1 : 0;
  a.a_blocked = (extra->flags & DFD_GEMM_A_BLOCKED) ? 1 : 0;
  a.pair = a.c_blocked | a.a_blocked;
  DFD_REQUIRE(epilogue != DFD_EPI_QKV_EXPORT || !extra->k_export == !extra->v_export, "dfd_gemm: QKV_EXPORT needs both k_export and v_export or neither");
  if (epilogue == DFD_EPI_RESIDUAL_POS && extra->drop_rng && extra->drop_p > 0.f) {
    DFD_REQUIRE(extra->drop_p < 1.f, "dfd_gemm: drop_p=%f", (double)extra->drop_p);
    const dfd_dropout_t dd{extra->drop_rng, extra->drop_site, extra->drop_p};
    a.drop = dfd_make_drop(&dd);
  }
  return DFD_OK;
}

static thread_local int g_gemm_variant = 0;
static thread_local int g_pair_variant = 0;

// What dfd_gemm (`who`; ab_dtype F32 / BF16) and dfd_gemm_fp8 (FP8) refuse about the numbers of a call, then the plan for
// what they accept (kernel 0 for M == 0: nothing to launch), or the refusal in the entry point's words.  Shared with the
// dfd_gemm_plan hook, so it reads `ptrs` and never a pointer.  n_cu <= 0: the current device's.
static int checked_plan(GemmPlan* p, const char* who, GemmArgs& a, GemmPtrs ptrs, int ab_dtype, int c_dtype, int epilogue, int n_cu) {
  const bool f8 = ab_dtype == DFD_FP8;
  DFD_REQUIRE(a.M >= 0 && a.N > 0 && a.K > 0, "%s: bad shape M=%lld N=%d K=%d", who, (long long)a.M, a.N, a.K);
  if (f8) {
    DFD_REQUIRE(c_dtype == DFD_BF16 || c_dtype == DFD_FP8, "%s: c_dtype=%d", who, c_dtype);
    DFD_REQUIRE(epilogue == DFD_EPI_BIAS || epilogue == DFD_EPI_BIAS_QUICKGELU || epilogue == DFD_EPI_BIAS_GELU || epilogue == DFD_EPI_QKV_EXPORT,
                "%s: epilogue %d not served (BIAS, BIAS_QUICKGELU, BIAS_GELU, QKV_EXPORT)", who, epilogue);
    DFD_REQUIRE(c_dtype == DFD_BF16 || (epilogue != DFD_EPI_QKV_EXPORT && a.out_inv_scale > 0.f), "%s: fp8 output needs out_inv_scale > 0 and a plain / QuickGELU / GELU epilogue", who);
    DFD_REQUIRE(a.lda >= a.K && a.ldw >= a.K && a.ldc >= a.N, "%s: leading dimensions", who);
  } else {
    DFD_REQUIRE(ab_dtype == DFD_F32 || ab_dtype == DFD_BF16, "%s: ab_dtype=%d", who, ab_dtype);
    DFD_REQUIRE(c_dtype == DFD_F32 || c_dtype == DFD_BF16, "%s: c_dtype=%d", who, c_dtype);
    DFD_REQUIRE(!(ab_dtype == DFD_F32 && c_dtype == DFD_BF16), "%s: f32 operands with bf16 output unsupported", who);
    DFD_REQUIRE(a.K % 32 == 0, "%s: K=%d must be a multiple of 32", who, a.K);
    const int esz = ab_dtype == DFD_F32 ? 4 : 2;
    DFD_REQUIRE(a.lda >= a.K && a.ldw >= a.K && (a.lda * esz) % 16 == 0 && (a.ldw * esz) % 16 == 0, "%s: lda=%lld ldw=%lld must be >= K and 16-byte multiples", who,
                (long long)a.lda, (long long)a.ldw);
    DFD_REQUIRE(!(ptrs.misaligned & (DFD_GEMM_PTR_A | DFD_GEMM_PTR_W)), "%s: A and W must be 16-byte aligned", who);
  }
  // epilogue-specific arguments
  const bool has_pos = ptrs.present & DFD_GEMM_PTR_POS;
  if (epilogue == DFD_EPI_PATCH_EMBED) {
    DFD_REQUIRE(has_pos && (ptrs.present & DFD_GEMM_PTR_CLS) && a.tokens > 1, "%s: PATCH_EMBED needs extra.pos, extra.cls, extra.tokens", who);
    DFD_REQUIRE(a.M % (a.tokens - 1) == 0, "%s: PATCH_EMBED M=%lld is not a whole number of frames", who, (long long)a.M);
    DFD_REQUIRE(c_dtype == DFD_F32 && a.ldc >= a.N, "%s: PATCH_EMBED writes an f32 token matrix", who);
  } else {
    DFD_REQUIRE(a.ldc >= a.N, "%s: ldc=%lld < N", who, (long long)a.ldc);
  }
  if (epilogue == DFD_EPI_QKV_EXPORT) {
    DFD_REQUIRE(a.tokens > 1 && (a.qkv_first == 0 || a.qkv_first == 1) && a.N % (3 - a.qkv_first) == 0,
                "%s: QKV_EXPORT needs extra.tokens, qkv_first in {0, 1} and N a multiple of the column blocks present", who);
    DFD_REQUIRE(a.M % a.tokens == 0, "%s: QKV_EXPORT M=%lld is not a whole number of frames", who, (long long)a.M);
    DFD_REQUIRE(!has_pos || a.frames_per_clip > 0, "%s: QKV_EXPORT with pos needs frames_per_clip", who);
  }
  if (epilogue == DFD_EPI_RESIDUAL_POS) {
    DFD_REQUIRE(a.tokens > 1, "%s: RESIDUAL_POS needs extra.tokens (patches per frame + 1)", who);
    DFD_REQUIRE(!has_pos || a.frames_per_clip > 0, "%s: RESIDUAL_POS with pos needs frames_per_clip", who);
  }
  DFD_REQUIRE(a.tile_rows == 0 || a.tile_rows == 224 || a.tile_rows == 256, "%s: tile blocks must be 0, 7 or 8", who);
  if (a.frames_per_clip < 1) a.frames_per_clip = 1;
  if (a.M == 0) {
    *p = GemmPlan{};
    return DFD_OK;
  }
  *p = gemm_plan(a, ptrs, ab_dtype, c_dtype, epilogue, g_gemm_variant, g_pair_variant, n_cu > 0 ? n_cu : dfd_cu_count());
  if (p->refused) {
    dfd_set_error("%s: %s%s (epilogue %d, M=%lld N=%d K=%d)", who,
                  a.pair ? "DFD_GEMM_C_BLOCKED / DFD_GEMM_A_BLOCKED: the ping-pong kernel does not serve this call: " : "call not served: ", p->refused,
                  epilogue, (long long)a.M, a.N, a.K);
    return DFD_ERR_INVALID_ARG;
  }
  if (p->tiles.grid == 0) {
    dfd_set_error("%s: cannot query the device", who);
    return DFD_ERR_LAUNCH;
  }
  return DFD_OK;
}

// Which kernel served this thread's last successful call; dfd_gemm_last_path is dfd_gemm's share of it, in its own numbers
static thread_local int g_last_kernel = 0;
static thread_local int g_last_path = 0;
extern "C" int dfd_gemm_last_kernel(void) { return g_last_kernel; }
extern "C" int dfd_gemm_last_path(void) { return g_last_path; }
extern "C" int dfd_gemm_set_variant(int variant) {
  const int old = g_gemm_variant;
  g_gemm_variant = variant;
  return old;
}

// ---- the c_fc -> c_proj pair with a fragment-blocked intermediate (gemm_blocked.hpp; hooks: include/dfdclip_hooks.h) ----
static thread_local int64_t g_pair_launches = 0;
extern "C" int dfd_gemm_pair_set_variant(int variant) {
  const int old = g_pair_variant;
  g_pair_variant = variant;
  return old;
}
extern "C" int64_t dfd_gemm_pair_launches(void) { return g_pair_launches; }
// Both halves are put to gemm_plan as the flagged calls of dense bf16 matrices with every pointer aligned, so the pair's
// plan cannot promise what dfd_gemm refuses (under the skip-the-ping-pong variant of dfd_gemm_set_variant, say, which leaves
// no kernel that knows the layout).  What it adds is policy: below 1,024 rows the pair stays with the kernels that serve
// small M (variant 2 waives that, for tests).
extern "C" int dfd_gemm_pair_plan(int64_t M, int D, int H) {
  if (g_pair_variant == 1 || M < 1 || D < 1 || H < 1) return 0;
  if (M < 1024 && g_pair_variant != 2) return 0;
  GemmArgs fc{}, pr{};
  fc.M = pr.M = M; fc.pair = pr.pair = 1;
  fc.N = H; fc.K = D; fc.lda = D; fc.ldw = D; fc.ldc = H; fc.c_blocked = 1;
  pr.N = D; pr.K = H; pr.lda = H; pr.ldw = H; pr.ldc = D; pr.a_blocked = 1;
  const GemmPtrs dense{DFD_GEMM_PTR_A | DFD_GEMM_PTR_W | DFD_GEMM_PTR_C | DFD_GEMM_PTR_BIAS, 0u};
  // (QuickGELU and the erf GELU share every rule that depends on the epilogue; the kernel does not depend on the CU count)
  auto blocked = [&](const GemmArgs& a, int epi) {
    return gemm_plan(a, dense, DFD_BF16, DFD_BF16, epi, g_gemm_variant, g_pair_variant, 256).kernel == DFD_GEMM_PINGPONG;
  };
  return blocked(fc, DFD_EPI_BIAS_QUICKGELU) && blocked(pr, DFD_EPI_BIAS) ? 1 : 0;
}

// validate -> plan -> the planned kernel's launcher -> record
static int plan_and_launch(const char* who, GemmArgs& a, int ab_dtype, int c_dtype, int epilogue, void* stream) {
  GemmPlan p;
  if (const int rc = checked_plan(&p, who, a, gemm_ptrs(a), ab_dtype, c_dtype, epilogue, 0)) return rc;
  if (p.kernel == 0) return DFD_OK;  // M == 0
  a.c_blocked = p.c_blocked;
  a.a_blocked = p.a_blocked;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool f8 = ab_dtype == DFD_FP8, cf8 = c_dtype == DFD_FP8;
  int rc, path;
  switch (p.kernel) {
    case DFD_GEMM_PINGPONG: rc = dfd_gemm256e_launch(p, a, f8, cf8, st); path = 257; break;
    case DFD_GEMM_PERSISTENT: rc = dfd_gemm256p_launch(p, a, f8, cf8, st); path = 256; break;
    case DFD_GEMM_TILE: rc = dfd_gemm256_launch(p, a, c_dtype, st); path = 256; break;
    default:  // DFD_GEMM_GENERAL
      rc = ab_dtype == DFD_F32 ? launch_gemm128<float, float>(p, a, st)
           : c_dtype == DFD_BF16 ? launch_gemm128<bf16_t, bf16_t>(p, a, st) : launch_gemm128<bf16_t, float>(p, a, st);
      path = 128;
  }
  if (rc != DFD_OK) return rc;
  g_last_kernel = p.kernel;
  if (!f8) g_last_path = path;  // (dfd_gemm_last_path reports dfd_gemm's launches only)
  if (p.c_blocked || p.a_blocked) ++g_pair_launches;
  return DFD_OK;
}

extern "C" int dfd_gemm_plan(int ab_dtype, int c_dtype, int epilogue, int64_t M, int N, int K, int64_t lda, int64_t ldw, int64_t ldc,
                             uint32_t flags, int tokens, int frames_per_clip, int qkv_first, unsigned has, unsigned misaligned, int n_cu,
                             dfd_gemm_plan_t* out) {
  dfd_gemm_extra extra{};
  extra.tokens = tokens; extra.frames_per_clip = frames_per_clip; extra.qkv_first = qkv_first; extra.flags = flags;
  GemmArgs a{};
  a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.out_inv_scale = 1.f;
  (void)fill_extra(a, epilogue, &extra);
  const unsigned optional = DFD_GEMM_PTR_EXPORT | DFD_GEMM_PTR_POS | DFD_GEMM_PTR_RESIDUAL;
  GemmPtrs ptrs{((2u * DFD_GEMM_PTR_EXPORT - 1u) & ~optional) | (has & optional), 0u};
  ptrs.misaligned = misaligned & ptrs.present;
  GemmPlan p;
  if (checked_plan(&p, ab_dtype == DFD_FP8 ? "dfd_gemm_fp8" : "dfd_gemm", a, ptrs, ab_dtype, c_dtype, epilogue, n_cu) != DFD_OK) return -1;
  if (out)
    *out = dfd_gemm_plan_t{p.kernel, p.epilogue, p.tiles.rows, p.tiles.tiles_m, p.tiles.ntiles, (uint32_t)p.tiles.grid, p.grid_y, p.block,
                           p.c_blocked, p.a_blocked, p.dynamic};
  return p.kernel;
}

extern "C" int dfd_gemm(const void* A, int64_t lda, const void* W, int64_t ldw, int ab_dtype, void* C, int64_t ldc,
                        int c_dtype, const float* bias, int epilogue, const dfd_gemm_extra* extra, int64_t M, int N,
                        int K, void* stream) {
  DFD_REQUIRE(A && W && C, "dfd_gemm: null pointer");
  DFD_REQUIRE(ab_dtype != DFD_FP8, "dfd_gemm: ab_dtype=%d", ab_dtype);  // (dfd_gemm_fp8's operands)
  GemmArgs a{};
  a.A = A; a.W = W; a.C = C; a.bias = bias;
  a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
  if (const int rc = fill_extra(a, epilogue, extra)) return rc;
  return plan_and_launch("dfd_gemm", a, ab_dtype, c_dtype, epilogue, stream);
}

extern "C" int dfd_gemm_fp8(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int c_dtype,
                            const float* col_scale, const float* bias, float out_inv_scale, int epilogue,
                            const dfd_gemm_extra* extra, int64_t M, int N, int K, void* stream) {
  DFD_REQUIRE(A && W && C && col_scale, "dfd_gemm_fp8: null pointer");
  GemmArgs a{};
  a.A = A; a.W = W; a.C = C; a.bias = bias; a.col_scale = col_scale; a.out_inv_scale = out_inv_scale;
  a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
  if (const int rc = fill_extra(a, epilogue, extra)) return rc;
  return plan_and_launch("dfd_gemm_fp8", a, DFD_FP8, c_dtype, epilogue, stream);
}

// gemm_tn.hip: bf16 operands read through the transposing LDS load, no HBM transposes
bool dfd_gemm_tn_supported(const void* A, int64_t lda, const void* B, int64_t ldb, int Ma, int Nb);
int dfd_gemm_tn_splits(int64_t R, int Ma, int Nb);
int dfd_gemm_tn_launch(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t R, int Ma, int Nb,
                       float* slabs, hipStream_t st, int* tile);

// which kernels served this thread's last successful dfd_gemm_at_b (include/dfdclip_hooks.h)
static thread_local int g_at_b_last_path = 0;
extern "C" int dfd_gemm_at_b_last_path(void) { return g_at_b_last_path; }

extern "C" size_t dfd_gemm_at_b_workspace(int64_t R, int Ma, int Nb, int dtype) {
  if (R <= 0 || Ma <= 0 || Nb <= 0) return 0;
  int64_t Rp;
  int splits;
  at_b_plan(R, Ma, Nb, &Rp, &splits);
  const size_t esz = dtype == DFD_F32 ? 4 : 2;
  size_t bytes = (size_t)(Ma + Nb) * Rp * esz;
  bytes = (bytes + 255) / 256 * 256;
  bytes += (size_t)splits * Ma * Nb * sizeof(float) + 256;
  if (dtype == DFD_BF16 && Ma % 128 == 0 && Nb % 128 == 0) {
    const size_t tn = (size_t)dfd_gemm_tn_splits(R, Ma, Nb) * Ma * Nb * sizeof(float) + 256;
    if (tn > bytes) bytes = tn;
  }
  return bytes;
}

extern "C" int dfd_gemm_at_b(const void* A, int64_t lda, const void* B, int64_t ldb, int dtype, float* C, int64_t R, int Ma,
                             int Nb, void* workspace, void* stream) {
  DFD_REQUIRE(A && B && C && workspace, "dfd_gemm_at_b: null pointer");
  DFD_REQUIRE(R > 0 && Ma > 0 && Nb > 0 && lda >= Ma && ldb >= Nb, "dfd_gemm_at_b: bad shape");
  DFD_REQUIRE(R < (int64_t)1 << 31, "dfd_gemm_at_b: R too large");
  DFD_REQUIRE(dtype == DFD_F32 || dtype == DFD_BF16, "dfd_gemm_at_b: dtype=%d", dtype);
  const bool tn = dtype == DFD_BF16 && dfd_gemm_tn_supported(A, lda, B, ldb, Ma, Nb);
  // the fallback's transposes put one block of 32 rows on grid.y (gemm_tn.hip puts the rows on no grid axis)
  DFD_REQUIRE(tn || (R + 31) / 32 <= 65535, "dfd_gemm_at_b: R=%lld needs more than the 65535 grid.y blocks of 32 rows the transpose path can launch",
              (long long)R);
  DFD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "dfd_gemm_at_b: workspace must be 256-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (tn) {
    int tile = 0;
    const int rc = dfd_gemm_tn_launch(A, lda, B, ldb, C, R, Ma, Nb, static_cast<float*>(workspace), st, &tile);
    if (rc == DFD_OK) g_at_b_last_path = tile;
    return rc;
  }
  const int rc = dtype == DFD_F32 ? launch_at_b<float>(A, lda, B, ldb, C, R, Ma, Nb, workspace, st)
                                  : launch_at_b<bf16_t>(A, lda, B, ldb, C, R, Ma, Nb, workspace, st);
  if (rc == DFD_OK) g_at_b_last_path = 1;
  return rc;
}
