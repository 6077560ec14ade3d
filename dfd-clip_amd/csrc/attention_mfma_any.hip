// Streaming bf16 MFMA self-attention for the encoder at ANY token count >= 33: out = softmax(q kᵀ · scale) v per
// (frame, head), head_dim 64 (reference clip/model.py:188-195).  attention_mfma.hip keeps all 32*NB scores of a query in
// registers, which ends at NB = 9 (288 tokens); here the keys are walked in chunks of 128 with an online softmax, so
// neither LDS nor the register file bounds the token count (ViT-L/14@336px: 577 tokens, DINOv2 at 518 px: 1370).
//
// One 256-thread workgroup (4 waves; two workgroups per CU) per (frame, head, span of 128 queries); wave w owns the
// 32-query block w of the span.  The spans of one (frame, head) are neighbours in the grid, so the K and V rows they
// all walk are read from HBM once and from L2 after that.
//   * Keys go through LDS in chunks of 4 key blocks (128 keys), double-buffered [K0][V0][K1][V1], 16 KB per image:
//     K row-major with 16-byte chunk c of row r at c ^ ((r >> 1) & 7), V as the row image that attn_read_v()
//     (attention_common.hpp) reads with the transposing LDS read.  Staging is plain: the global loads of chunk c+1 are
//     issued before the arithmetic of chunk c, land in registers, and are written to the other buffer behind it; one
//     __syncthreads() per chunk.  No LDS-DMA, no counted waits.
//   * Per chunk: Sᵀ = K·Qᵀ with v_mfma_f32_32x32x16_bf16 (lane = query column, 64 score registers), chunk max,
//     m' = max(m, chunk max), alpha = exp2((m − m')·scale·log2 e); l and both O tiles are rescaled by alpha, the
//     exponentials — converted pairwise to bf16 — are the B operand of Oᵀ += Vᵀ·Pᵀ (accumulator-as-operand).
//   * Pad keys (>= tokens, last chunk only) score −inf before the max and their K and V rows are ZERO in LDS (0 · NaN
//     from stale LDS would be NaN).  Chunks are 0 .. ceil(tokens / 128) − 1, so every chunk has a live key and the
//     first one makes m finite before the first alpha (exp2(−inf) = 0 scales the zero start state).
//   * Query rows past the frame are clamped on load and never stored; a wave whose whole block is past the frame only
//     stages and waits at the barriers.  Output leaves as 8-byte pieces (4 channels of one query per register group).
// The result of a query depends on its frame's rows alone: not on n_frames, the grid or the CU.
#include "attention_common.hpp"

namespace {

constexpr int ANY_CB = 4;                // key blocks per chunk
constexpr int ANY_CK = ANY_CB * 32;      // keys per chunk
constexpr int ANY_IMG = ANY_CK * 128;    // bytes of one K or V image
constexpr int ANY_SPAN = 128;            // queries per workgroup
constexpr int ANY_IT = ANY_CK * 8 / 256; // 16-byte pieces of an image per thread

__global__ __launch_bounds__(256, 2) void attn_mfma_any_kernel(const bf16_t* __restrict__ qkv, int64_t ld_qkv,
                                                               bf16_t* __restrict__ out, int64_t ld_out, int tokens, int heads,
                                                               int spans, float scale_log2e) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * ANY_IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int item = blockIdx.x / spans, span = blockIdx.x - item * spans;
  const int frame = item / heads, head = item - frame * heads;
  const int D = heads * HD;
  const bf16_t* base = qkv + (int64_t)frame * tokens * ld_qkv + head * HD;

  bf16x8 kreg[ANY_IT], vreg[ANY_IT];
  auto load_kv = [&](int chunk) {
#pragma unroll
    for (int it = 0; it < ANY_IT; ++it) {
      const int c = tid + it * 256;
      const int key = chunk * ANY_CK + (c >> 3), ch = c & 7;
      const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      kreg[it] = z;
      vreg[it] = z;
      if (key < tokens) {
        const bf16_t* src = base + (int64_t)key * ld_qkv + ch * 8;
        kreg[it] = *reinterpret_cast<const bf16x8*>(src + D);
        vreg[it] = *reinterpret_cast<const bf16x8*>(src + 2 * D);
      }
    }
  };
  auto write_kv = [&](unsigned char* Kb) {
#pragma unroll
    for (int it = 0; it < ANY_IT; ++it) {
      const int c = tid + it * 256;
      const int kl = c >> 3, ch = c & 7;
      *reinterpret_cast<bf16x8*>(Kb + kl * 128 + ((ch ^ ((kl >> 1) & 7)) << 4)) = kreg[it];
      *reinterpret_cast<bf16x8*>(Kb + ANY_IMG + kl * 128 + ((ch ^ (((kl >> 1) & 1) << 2)) << 4)) = vreg[it];
    }
  };

  const int q0 = span * ANY_SPAN + wave * 32;
  const bool active = q0 < tokens;  // wave-uniform
  const int q = q0 + r;
  bf16x8 qf[4];
  {
    const int qc = q < tokens ? q : tokens - 1;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(base + (int64_t)qc * ld_qkv + s * 16 + h * 8);
  }
  load_kv(0);
  write_kv(smem);
  __syncthreads();

  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 O[2] = {zero16, zero16};
  float m = -INFINITY, l = 0.f;
  const int ksw = (r >> 1) & 7;
  const int nchunks = (tokens + ANY_CK - 1) / ANY_CK;
  for (int c = 0; c < nchunks; ++c) {
    const unsigned char* Ks = smem + (c & 1) * 2 * ANY_IMG;
    const unsigned char* Vs = Ks + ANY_IMG;
    const bool more = c + 1 < nchunks;
    if (more) load_kv(c + 1);  // in flight during this chunk's arithmetic
    if (active) {
      // ---- Sᵀ[key][q] of the chunk; K fragments read one d-slice ahead of their MFMAs -------------------
      f32x16 S[ANY_CB];
      bf16x8 kfa[ANY_CB], kfb[ANY_CB];
      auto read_k = [&](bf16x8 (&kf)[ANY_CB], int s) {
#pragma unroll
        for (int kb = 0; kb < ANY_CB; ++kb)
          kf[kb] = *reinterpret_cast<const bf16x8*>(Ks + (kb * 32 + r) * 128 + (((2 * s + h) ^ ksw) << 4));
      };
      auto mma_k = [&](const bf16x8 (&kf)[ANY_CB], int s) {
#pragma unroll
        for (int kb = 0; kb < ANY_CB; ++kb)
          S[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kb], qf[s], s == 0 ? zero16 : S[kb], 0, 0, 0);
      };
      read_k(kfa, 0);
      __builtin_amdgcn_sched_barrier(0);
      read_k(kfb, 1);
      mma_k(kfa, 0);
      __builtin_amdgcn_sched_barrier(0);
      read_k(kfa, 2);
      mma_k(kfb, 1);
      __builtin_amdgcn_sched_barrier(0);
      read_k(kfb, 3);
      mma_k(kfa, 2);
      __builtin_amdgcn_sched_barrier(0);
      mma_k(kfb, 3);
      __builtin_amdgcn_sched_barrier(0);
      if (!more) {  // only the last chunk holds keys >= tokens
#pragma unroll
        for (int kb = 0; kb < ANY_CB; ++kb)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = c * ANY_CK + kb * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (key >= tokens) S[kb][e] = -INFINITY;
          }
      }
      // ---- online softmax: registers + one exchange with lane ^ 32 per reduction -------------------------
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < ANY_CB; ++kb)
#pragma unroll
        for (int e = 0; e < 16; e += 2) mx = vmax3(mx, S[kb][e], S[kb][e + 1]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m, mx);
      const float alpha = __builtin_amdgcn_exp2f((m - m_new) * scale_log2e);
      m = m_new;
      float sl2 = scale_log2e;
      float nmc = -m_new * scale_log2e;
      asm volatile("" : "+s"(sl2));  // opaque scalar: the vector expression below packs into v_pk_fma_f32
      f32x16 lv = zero16;
#pragma unroll
      for (int kb = 0; kb < ANY_CB; ++kb) {
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const f32x2v t = __builtin_elementwise_fma(f32x2v{S[kb][e], S[kb][e + 1]}, f32x2v{sl2, sl2}, f32x2v{nmc, nmc});
          S[kb][e] = __builtin_amdgcn_exp2f(t[0]);
          S[kb][e + 1] = __builtin_amdgcn_exp2f(t[1]);
        }
        lv += S[kb];
      }
      float cs = ((lv[0] + lv[1]) + (lv[2] + lv[3])) + ((lv[4] + lv[5]) + (lv[6] + lv[7])) +
                 (((lv[8] + lv[9]) + (lv[10] + lv[11])) + ((lv[12] + lv[13]) + (lv[14] + lv[15])));
      cs += __shfl_xor(cs, 32, 64);
      l = l * alpha + cs;
      O[0] *= alpha;
      O[1] *= alpha;
      // ---- Oᵀ[d][q] += Σ_key V[key][d] · Pᵀ[key][q]; V fragments read one 16-key step ahead ----------------
      auto mma_v = [&](const bf16x8 (&vf)[2], int step) {
        const int kb = step >> 1, sl = step & 1;
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = (bf16_t)S[kb][8 * sl + j];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) O[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[dt], pf, O[dt], 0, 0, 0);
      };
      bf16x8 vfa[2], vfb[2];
      attn_read_v(vfa, Vs, lane, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int step = 0; step < 2 * ANY_CB; step += 2) {
        attn_read_v(vfb, Vs, lane, step + 1);
        mma_v(vfa, step);
        __builtin_amdgcn_sched_barrier(0);
        if (step + 2 < 2 * ANY_CB) attn_read_v(vfa, Vs, lane, step + 2);
        mma_v(vfb, step + 1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (more) write_kv(smem + ((c + 1) & 1) * 2 * ANY_IMG);  // that buffer was last read in chunk c-1, a barrier ago
    __syncthreads();
  }

  if (active && q < tokens) {
    const float inv = 1.0f / l;
    bf16_t* op = out + ((int64_t)frame * tokens + q) * ld_out + head * HD;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16_t)(O[dt][4 * g + e] * inv);
        *reinterpret_cast<bf16x4*>(op + dt * 32 + 8 * g + 4 * h) = o;
      }
  }
}

}  // namespace

int dfd_attn_launch_stream(const AttnPlan& p, const AttnCall& c) {
  static_assert(ANY_SPAN == ATTN_STREAM_SPAN, "the plan's grid counts the kernel's spans");
  const int spans = (c.tokens + ANY_SPAN - 1) / ANY_SPAN;
  return attn_launch<&attn_mfma_any_kernel>("dfd_attention_fwd(mfma, streaming)", p, c.st, static_cast<const bf16_t*>(c.qkv), c.ld_qkv,
                                            static_cast<bf16_t*>(c.out), c.ld_out, c.tokens, c.heads, spans, c.scale * 1.4426950408889634f);
}
