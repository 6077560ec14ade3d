// Pieces shared by the persistent encoder-attention kernels (attention_mfma.hip: 193..224 tokens, loader wave;
// attention_mfma_xrow.hip: 257 tokens, eight query blocks + one extra row): LDS images and their LDS-DMA staging, the
// register softmax and the second product.  head_dim 64 everywhere (reference clip/model.py:188-195).
// At the end, the host side of the whole family behind dfd_attention_fwd: which kernel serves a call (attn_plan), the one
// launcher, and the launch functions its four files export.
#pragma once
#include "common.hpp"
#include "../../include/dfdclip_hooks.h"

namespace {

constexpr int HD = 64;

typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef short short4v __attribute__((ext_vector_type(4)));
typedef int v4i_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float vmax3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// LDS-DMA in 1 KB pieces (8 rows): lane (sub = lane >> 3, pos = lane & 7) moves 16-byte chunk pos^swizzle of row
// 8*piece + sub; the swizzle of the K and Q images, ((row >> 1) & 7), depends on the piece only through its parity.
// attn_stage_k / _v issue pieces p0, p0 + dp, .. < np (every piece has live lanes): all of them from a loader wave
// (p0 = 0, dp = 1), or every eighth when the eight compute waves share the job (dp even: one parity per wave).
__device__ __forceinline__ void attn_stage_k(__amdgpu_buffer_rsrc_t srd, unsigned char* kimg, uint32_t sbase, uint32_t ldq,
                                             uint32_t Db, int lane, int np, int tokens, int p0 = 0, int dp = 1) {
  const int sub = lane >> 3, pos = lane & 7;
  const uint32_t row0 = (uint32_t)sub * ldq;
  const uint32_t k_even = row0 + Db + ((pos ^ ((sub >> 1) & 3)) << 4), k_odd = row0 + Db + ((pos ^ (((sub >> 1) & 3) | 4)) << 4);
  for (int p = p0; p < np; p += dp) {
    if (8 * p + sub < tokens)  // lanes past the image write nothing
      __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (lds_ptr_t)(kimg + p * 1024), 16, ((p & 1) ? k_odd : k_even) + p * 8 * ldq, sbase, 0, 0);
  }
}
__device__ __forceinline__ void attn_stage_v(__amdgpu_buffer_rsrc_t srd, unsigned char* vimg, uint32_t sbase, uint32_t ldq,
                                             uint32_t Db, int lane, int np, int tokens, int p0 = 0, int dp = 1) {
  const int sub = lane >> 3, pos = lane & 7;
  const uint32_t v_any = (uint32_t)sub * ldq + 2 * Db + ((pos ^ (((sub >> 1) & 1) << 2)) << 4);
  for (int p = p0; p < np; p += dp) {
    if (8 * p + sub < tokens)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (lds_ptr_t)(vimg + p * 1024), 16, v_any + p * 8 * ldq, sbase, 0, 0);
  }
}

// ---- softmax over the key axis of Sᵀ[key][q] (lane = query column; key of element e of block kb, lane half h:
// 32 kb + (e & 3) + 8 (e >> 2) + 4 h): registers + one exchange with lane ^ 32.  Returns the row sum; S holds the
// exponentials.  SHORT: the last block has at most 8 keys, so only its elements 0..3 can be live — the other twelve are
// not exponentiated (elements 4..7 are cleared for the one step of the second product that still runs).
// The softmax is the VALU-bound part of these kernels (two waves per SIMD): v_max3 without the NaN canonicalisation
// fmaxf() drags in, packed f32 multiply-add and packed row sums.
struct AttnNoTick {
  __device__ __forceinline__ void operator()(int) const {}
};
// tick(kb) runs behind the exponentials of block kb (a kernel without a loader wave spreads its LDS-DMA there).
template <int NB, bool SHORT, typename Tick = AttnNoTick>
__device__ __forceinline__ float attn_softmax(f32x16 (&S)[NB], int tokens, int h, float scale_log2e, Tick tick = Tick()) {
  constexpr int LE = SHORT ? 4 : 16;
#pragma unroll
  for (int e = 0; e < LE; ++e) {
    const int key = (NB - 1) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
    if (key >= tokens) S[NB - 1][e] = -INFINITY;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb)
#pragma unroll
    for (int e = 0; e < (kb == NB - 1 ? LE : 16); e += 2) mx = vmax3(mx, S[kb][e], S[kb][e + 1]);
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sl2 = scale_log2e;
  float nmc = -mx * scale_log2e;
  asm volatile("" : "+s"(sl2));  // opaque scalars: the vector expression below packs into v_pk_fma_f32
  f32x16 lv;
#pragma unroll
  for (int e = 0; e < 16; ++e) lv[e] = 0.f;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
    for (int e = 0; e < (kb == NB - 1 ? LE : 16); e += 2) {
      const f32x2v t = __builtin_elementwise_fma(f32x2v{S[kb][e], S[kb][e + 1]}, f32x2v{sl2, sl2}, f32x2v{nmc, nmc});
      S[kb][e] = __builtin_amdgcn_exp2f(t[0]);
      S[kb][e + 1] = __builtin_amdgcn_exp2f(t[1]);
    }
    if (SHORT && kb == NB - 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) lv[e] += S[kb][e];
#pragma unroll
      for (int e = 4; e < 8; ++e) S[kb][e] = 0.f;
    } else {
      lv += S[kb];
    }
    tick(kb);
  }
  float l = ((lv[0] + lv[1]) + (lv[2] + lv[3])) + ((lv[4] + lv[5]) + (lv[6] + lv[7])) +
            (((lv[8] + lv[9]) + (lv[10] + lv[11])) + ((lv[12] + lv[13]) + (lv[14] + lv[15])));
  l += __shfl_xor(l, 32, 64);
  return l;
}

// ---- V operand of Oᵀ[d][q] = Σ_key V[key][d] · Pᵀ[key][q] for one 16-key step, through the transposing LDS read.
// V image: [key][64] bf16, 16-byte chunk c of key k at position c ^ (((k >> 1) & 1) << 2).  Lane (r, h): d row r of
// tile dt, keys base + 4h + {0..3} and base + 8 + 4h + {0..3}; in its 16-lane group (d columns 16*(r>>4) ..), lane
// 4q+p supplies the address of key row q, d columns 4p..4p+3.
__device__ __forceinline__ void attn_read_v(bf16x8 (&vf)[2], const unsigned char* Vs, int lane, int step) {
  const int h = lane >> 5, tq = (lane & 15) >> 2, tp = lane & 3, rr = (lane >> 4) & 1;
  const int kbase = (step >> 1) * 32 + 16 * (step & 1) + 4 * h + tq;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const int c = 4 * dt + 2 * rr + (tp >> 1);
    const int k1 = kbase, k2 = kbase + 8;
    const unsigned char* a1 = Vs + k1 * 128 + ((c ^ (((k1 >> 1) & 1) << 2)) << 4) + 8 * (tp & 1);
    const unsigned char* a2 = Vs + k2 * 128 + ((c ^ (((k2 >> 1) & 1) << 2)) << 4) + 8 * (tp & 1);
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)a1);
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4v __attribute__((address_space(3)))*)a2);
    short8 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
    vf[dt] = __builtin_bit_cast(bf16x8, v);
  }
}

// The second product over all 16-key steps with a live key; the P operand comes straight out of the S registers
// (accumulator-as-operand, converted pairwise to bf16), V fragments are read one step ahead of the MFMAs that use them.
struct AttnNoRider {
  __device__ __forceinline__ void operator()(const bf16x8 (&)[2], int) const {}
};
// rider(vf, step) runs behind the MFMAs of a step with the V fragments still in registers (a second, independent
// accumulation over the same V — the 257-token kernel's extra row).
template <int NB, bool SHORT, typename Rider = AttnNoRider>
__device__ __forceinline__ void attn_pv(const f32x16 (&S)[NB], const unsigned char* Vs, int lane, f32x16 (&O)[2], Rider rider = Rider()) {
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto mma_v = [&](const bf16x8 (&vf)[2], int step) {
    const int kb = step >> 1, sl = step & 1;
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 8; ++j) pf[j] = (bf16_t)S[kb][8 * sl + j];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[dt], pf, step == 0 ? zero16 : O[dt], 0, 0, 0);
  };
  bf16x8 vfa[2], vfb[2];
  attn_read_v(vfa, Vs, lane, 0);
  __builtin_amdgcn_sched_barrier(0);
  constexpr int NS = SHORT ? 2 * NB - 1 : 2 * NB;  // 16-key steps with a live key
#pragma unroll
  for (int step = 0; step < NS; step += 2) {
    if (step + 1 < NS) attn_read_v(vfb, Vs, lane, step + 1);
    mma_v(vfa, step);
    rider(vfa, step);
    __builtin_amdgcn_sched_barrier(0);
    if (step + 2 < NS) attn_read_v(vfa, Vs, lane, step + 2);
    if (step + 1 < NS) {
      mma_v(vfb, step + 1);
      rider(vfb, step + 1);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One 16-byte store per lane, scalar-offset field = 0.  With a REGISTER in that field the compiler's hazard recognizer
// leaves out the wait states it otherwise puts between a store of more than 8 bytes per lane and a VALU write of the
// store's data registers (LLVM, GCNHazardRecognizer::createsVALUHazard: "this hazard only exists if the instruction is not
// using a register in the soffset field") — and on gfx950 the store had not always read its data by then: it went out
// with the next instruction's result in its first data register for the lanes read last (round 3: 32 elements of a
// 32 x 64 tile, sporadically, more often on the second wave of a SIMD).  tools/isa_lint.py checks every kernel for it.
__device__ __forceinline__ void attn_store_line(v4i_t d, __amdgpu_buffer_rsrc_t srd, uint32_t off) {
  __builtin_amdgcn_raw_buffer_store_b128(d, srd, off, 0, 0);
}

template <int N> __device__ __forceinline__ void attn_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

}  // namespace

// ---- host: one launch plan for the five kernels behind dfd_attention_fwd ------------------------------------------------
// attn_plan is the only place that knows token windows, item thresholds, LDS budgets and 32-bit extents; its table is
// written out once, in include/dfdclip_hooks.h.  A new kernel or window is a path there, a row here, a case in its
// file's launcher and a row of the table in tests/test_abi_cpu.py.
enum AttnPath {  // 0: no call yet / no kernel
  ATTN_NONE = 0, ATTN_ROWS = DFD_ATTN_ROWS, ATTN_ROWS_CHUNKED = DFD_ATTN_ROWS_CHUNKED, ATTN_ITEM7 = DFD_ATTN_ITEM7,
  ATTN_ITEM9 = DFD_ATTN_ITEM9, ATTN_PERSIST7_SHORT = DFD_ATTN_PERSIST7_SHORT, ATTN_PERSIST7 = DFD_ATTN_PERSIST7,
  ATTN_XROW = DFD_ATTN_XROW, ATTN_STREAM = DFD_ATTN_STREAM
};

struct AttnPlan {
  int path;  // ATTN_NONE: the (frame, head) items do not fit the grid of the kernel that would serve the call
  unsigned grid, block;
  size_t lds;                     // dynamic LDS of the launch
  int chunk;                      // keys per staging chunk (ATTN_ROWS_CHUNKED), else 0
  uint32_t qkv_bytes, out_bytes;  // what the persistent kernels' buffer descriptors span, else 0
};

constexpr size_t ATTN_LDS_MAX = 160 * 1024;  // of a CU; a launch gets 64 KiB unasked
// LDS of the MFMA kernels (the per-item and the 257-token file assert that these are their layouts)
constexpr size_t attn_item_lds(int nb) { return (size_t)nb * 32 * 128 + 64 * ((size_t)nb * 64 + 8); }  // K rows, transposed V
constexpr size_t attn_persist_lds(int tokens, int nb) { return (size_t)4 * tokens * 128 + (size_t)2 * nb * 4096; }  // [K0][V0][K1][V1], 2 Q images per wave
constexpr size_t ATTN_XROW_LDS = 4 * 257 * 128 + 8 * 2048 + 2560;
constexpr int ATTN_STREAM_SPAN = 128;  // queries per workgroup of the streaming kernel

// variant: dfd_attention_set_variant; n_cu <= 0 (the device cannot be queried) reads as 256.  No HIP call, no pointer.
inline AttnPlan attn_plan(int dtype, int n_frames, int tokens, int heads, int64_t ld_qkv, int64_t ld_out, int variant, int n_cu) {
  const int64_t items = (int64_t)n_frames * heads, GRID_MAX = 0x7fffffff, EXTENT_MAX = 0xfffffff0;
  const size_t esz = dtype == DFD_F32 ? 4 : 2;
  auto per_item = [&](int path, size_t lds, int chunk) {  // one 256-thread workgroup per item
    return AttnPlan{items <= GRID_MAX ? path : ATTN_NONE, (unsigned)items, 256u, lds, chunk, 0u, 0u};
  };
  const int nb = (tokens + 31) / 32;  // the register kernels mask only their last key block: NB = ceil(tokens / 32) exactly
  if (dtype == DFD_BF16 && (nb == 7 || nb == 9)) {
    // persistent forms: enough items to fill the chip, a whole number of workgroups per XCD, offsets that fit 32 bits
    const int64_t last_row = (int64_t)n_frames * tokens - 1;
    const int64_t qkv_bytes = last_row * ld_qkv * 2 + (int64_t)3 * heads * 128, out_bytes = last_row * ld_out * 2 + (int64_t)heads * 128;
    const unsigned grid = (unsigned)(n_cu <= 0 ? 256 : n_cu) & ~7u;
    const size_t lds = nb == 7 ? attn_persist_lds(tokens, 7) : ATTN_XROW_LDS;
    if (items >= 512 && grid >= 8 && qkv_bytes <= EXTENT_MAX && out_bytes <= EXTENT_MAX && (nb == 7 ? lds <= ATTN_LDS_MAX : tokens == 257))
      return AttnPlan{nb == 9 ? ATTN_XROW : tokens <= 6 * 32 + 8 ? ATTN_PERSIST7_SHORT : ATTN_PERSIST7, grid, 512u, lds, 0,
                      (uint32_t)qkv_bytes, (uint32_t)out_bytes};
    return per_item(nb == 7 ? ATTN_ITEM7 : ATTN_ITEM9, attn_item_lds(nb), 0);
  }
  const int64_t spans = (tokens + ATTN_STREAM_SPAN - 1) / ATTN_STREAM_SPAN;
  if (dtype == DFD_BF16 && tokens > 32 && variant != 2 && items <= GRID_MAX / spans)
    return AttnPlan{ATTN_STREAM, (unsigned)(items * spans), 256u, 0, 0, 0u, 0u};
  // rows: whole-head staging wherever K and V of a head fit LDS; beyond that, chunks of 64 KiB (two workgroups per CU)
  const size_t whole = 2 * (size_t)tokens * 64 * esz;
  const int chunk = variant == 1 ? 16 : whole > ATTN_LDS_MAX ? (int)(64 * 1024 / (2 * 64 * esz)) : 0;
  return chunk > 0 ? per_item(ATTN_ROWS_CHUNKED, 2 * (size_t)chunk * 64 * esz, chunk) : per_item(ATTN_ROWS, whole, 0);
}

// Raise the kernel's dynamic-LDS limit the first time a launch of this instantiation asks for more than 64 KiB (once per
// process, to the CU's whole LDS: these kernels are launched 12-24 times per pass inside graph capture), launch, report.
template <auto Kernel, typename... A>
int attn_launch(const char* what, const AttnPlan& p, hipStream_t st, A... args) {
  static bool raised = false;
  if (p.lds > 64 * 1024 && !raised) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_LDS_MAX);
    raised = true;
  }
  hipLaunchKernelGGL(Kernel, dim3(p.grid), dim3(p.block), p.lds, st, args...);
  DFD_CHECK_LAUNCH(what);
  return DFD_OK;
}

// What dfd_attention_fwd hands to the file that holds the planned kernel.  Each file exports one launcher; none decides.
struct AttnCall {
  const void* qkv;
  int64_t ld_qkv;
  void* out;
  int64_t ld_out;
  int n_frames, tokens, heads;
  float scale;
  hipStream_t st;
};
int dfd_attn_launch_mfma(const AttnPlan& p, const AttnCall& c);    // attention_mfma.hip: ITEM7, ITEM9, PERSIST7_SHORT, PERSIST7
int dfd_attn_launch_xrow(const AttnPlan& p, const AttnCall& c);    // attention_mfma_xrow.hip: XROW
int dfd_attn_launch_stream(const AttnPlan& p, const AttnCall& c);  // attention_mfma_any.hip: STREAM
