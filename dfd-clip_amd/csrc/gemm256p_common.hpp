// Pieces shared by the two persistent GEMM kernels (gemm256e.hip: ping-pong K loop, tried first; gemm256p.hip: the K
// depths that one does not serve; each with a bf16 and an e4m3 form).  They differ in their K loops only.  Here: tile /
// ring geometry, the tile order, counted vmcnt waits, buffer descriptors, THE per-tile epilogue (tile_epilogue) and the
// host side (the planned launch of an instantiation; the plan itself is gemm_plan.hpp's).  A K step is 128 BYTES of every
// operand row (64 bf16 or 128 fp8 elements), so the LDS ring, the LDS-DMA pieces and the XOR swizzle are the same for both
// element types.
#pragma once
#include <type_traits>

#include "gemm_plan.hpp"

#include "gelu.hpp"
#include "gemm_blocked.hpp"

typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef v4i_t v4i;
typedef int v8i __attribute__((ext_vector_type(8)));

namespace {

// Output stores: non-temporal (aux bit 1) when the caller marks the output as streaming: it then goes past L2
// instead of evicting the operand panels the XCD's other workgroups are reading (c_fc 0.46 -> 0.41 ms).
__device__ __forceinline__ void store_out(v4i_t d, __amdgpu_buffer_rsrc_t srd, uint32_t off, int stream_out) {
  if (stream_out) {
    __builtin_amdgcn_raw_buffer_store_b128(d, srd, off, 0, 2);
  } else {
    __builtin_amdgcn_raw_buffer_store_b128(d, srd, off, 0, 0);
  }
}

constexpr int TM = 256, TN = 256, TK = 64;  // TM: rows of A staged per step; a tile USES 32*RB of them (RB = 8 or 7)
constexpr int ROWB = TK * 2;            // 128 B per LDS row = one cache line
constexpr int A_BYTES = TM * ROWB;      // 32 KB
constexpr int SLOT = (TM + TN) * ROWB;  // 64 KB
constexpr int RING = 2 * SLOT;          // 128 KB
constexpr int STAGE = 4096;             // per wave: 32 rows x 128 B
typedef __attribute__((address_space(3))) void* lds_ptr_t;

struct Tile {
  int m0, n0;
};

// tile order: column GROUPS of at most 6 tiles, inside a group row panel major / column minor (gemm256.hip)
__device__ __forceinline__ Tile decode_tile(int idx, int tiles_m, int tiles_n, int tile_rows) {
  const int ngroups = (tiles_n + 5) / 6;  // (group widths 2 .. 12 measure the same within 1 %; single columns lose 8-25 %)
  const int gcols = (tiles_n + ngroups - 1) / ngroups;
  int grp = idx / (tiles_m * gcols);
  grp = grp < ngroups - 1 ? grp : ngroups - 1;
  const int rem = idx - grp * tiles_m * gcols;
  const int cols_here = min(gcols, tiles_n - grp * gcols);
  const int tm = rem / cols_here, tn = grp * gcols + (rem - tm * cols_here);
  return Tile{tm * tile_rows, tn * TN};
}

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// The lane id as a value the compiler cannot see through: addresses rebuilt from it are recomputed where they are used
// instead of being hoisted out of the tile loop (and spilled)
__device__ __forceinline__ int opaque_lane() {
  int l = threadIdx.x & 63;
  asm volatile("" : "+v"(l));
  return l;
}

// XCD-aware, bijective position of this workgroup inside one round of the grid (blocks b and b+8 share an XCD): each XCD
// takes a contiguous run of the tile order every round
__device__ __forceinline__ int xcd_position() {
  const int G = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = G >> 3, r8 = G & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// buffer descriptors: ONE per matrix, 32-bit byte offsets per lane, out-of-range loads read 0 and stores are dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_srd(const void* p, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(uint32_t)bytes, 0x00020000);
}
// ... and as four plain words, for loads issued by inline asm
__device__ __forceinline__ v4i words(const float* p, int bytes) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  return v4i{(int)(uint32_t)u, (int)((uint32_t)(u >> 32) & 0xffffu), bytes, 0x00020000};
}
// (ABLK / CBLK: the instantiation can read A / write C fragment-blocked, where the launch's flag says so)
template <bool F8, bool CF8, bool ABLK = false, bool CBLK = false>
struct OperandSrds {
  __amdgpu_buffer_rsrc_t A, W, C;
  __device__ __forceinline__ explicit OperandSrds(const GemmArgs& a)
      : A(make_srd(a.A, rows(a.M, ABLK && a.a_blocked) * a.lda * (F8 ? 1 : 2))), W(make_srd(a.W, (int64_t)a.N * a.ldw * (F8 ? 1 : 2))),
        C(make_srd(a.C, rows(a.M, CBLK && a.c_blocked) * a.ldc * (CF8 ? 1 : 2))) {}
  // a fragment-blocked matrix (gemm_blocked.hpp) keeps whole row groups: the rows of the last one reach to a multiple of 16
  static __device__ __forceinline__ int64_t rows(int64_t M, bool blocked) { return blocked ? (M + 15) & ~(int64_t)15 : M; }
};
// The stores of a tile's epilogue that the wave may count in the next tile's first waits (gemm256e.hip's header has the
// reason): all of them if all of the wave's rows are inside M, else none.
template <int RB> __device__ __forceinline__ int countable_stores(int stores, const Tile& t, int wr, int64_t M) {
  return (int64_t)t.m0 + (wr + 1) * 16 * RB <= M ? stores : 0;
}

// ---- the per-tile epilogue: bias, activation, LDS-staged whole-line stores, left in flight ------------------------------
// acc: the wave's 16 RB x 64 block of tile `cur` (wave row wr, wave column wc); b4 / cs4: bias and (fp8) column scale of
// its 64 columns as accumulator fragments; ep: the wave's 4 KB of staging; D: columns per q / k / v block (QKV_EXPORT).
// Returns the number of stores the wave issued.  The caller has requested the next tile's first operands already, so
// that the stores drain under that tile's first K steps.
// Every address below is rebuilt from an opaque copy of the lane id: left to itself the compiler hoists two dozen
// tile-invariant address registers out of the tile loop and spills them (scratch traffic counts in vmcnt and would drain
// the stores these kernels exist to leave in flight).
// BLK: the instantiation also has the fragment-blocked form of the bf16 store (gemm_blocked.hpp), taken where
// a.c_blocked says so: no staging at all, each lane stores its own fragments.
template <int EPI, int RB, bool F8, bool CF8, bool BLK = false>
__device__ __forceinline__ int tile_epilogue(const GemmArgs& a, f32x4 (&acc)[RB][4], const f32x4 (&b4)[4], const f32x4 (&cs4)[4], unsigned char* const ep,
                                             const Tile& cur, int wr, int wc, int le, int D, __amdgpu_buffer_rsrc_t srdC) {
  constexpr int WROWS = 16 * RB;  // rows per wave
  const int er = le & 15, eq = le >> 4;          // accumulator fragment: row er of a 16-row block, columns 4*eq ..
  const int drow = le >> 3, dc = le & 7;         // drain: row drow of an 8-row group, 16-byte chunk dc
  const int nb = cur.n0 + wc * 64;
  const int64_t mrow0 = (int64_t)cur.m0 + wr * WROWS + drow;  // first row this lane stores
  const int rows_left = (int)min((int64_t)0x7fffffff, a.M - mrow0);
  int which = 0;
  if constexpr (EPI == DFD_EPI_QKV_EXPORT) which = cur.n0 / D + a.qkv_first;  // 0 = q, 1 = k, 2 = v
  const bool exporting = EPI == DFD_EPI_QKV_EXPORT && which > 0 && a.k_export != nullptr;
  int stores = 2 * RB;
  // (column scale and) bias once, in place: both copies of an exported tile read the same registers
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (F8) acc[i][j] = acc[i][j] * cs4[j] + b4[j];
      else acc[i][j] += b4[j];
    }
  if constexpr (EPI == DFD_EPI_QKV_EXPORT) {
    if (exporting) {
      // Exported copy of a K / V tile FIRST (its positional-embedding loads then wait only for loads, never for
      // this tile's stores): bf16(acc + bias + pos[frame % T]) -> row frame*(tokens-1) + token-1 of the export,
      // the CLS row dropped.  Eight sub-passes of 16 rows parked as f32 (4 KB); the drain adds the embedding
      // (two 16-byte loads per store, requested at the top of the sub-pass) and rounds once.
      stores = 4 * RB;
      const int ecol = nb - (which - a.qkv_first) * D + dc * 8;  // first of this lane's 8 export columns
      unsigned char* const parkf = ep + er * 256;                 // unit (j*4 + eq) ^ er of a 256-byte row
      // (descriptors of the export [frames * (tokens - 1), D] bf16 and of the embedding [T, D] f32, built here from the
      // arguments: three descriptors kept across the K loop cost the fp8 form of gemm256e.hip a spill)
      const int64_t erows = (a.M / a.tokens) * (a.tokens - 1);
      const __amdgpu_buffer_rsrc_t srdE = make_srd(which == 2 ? a.v_export : a.k_export, erows * D * 2);
      const __amdgpu_buffer_rsrc_t srdP = make_srd(a.pos ? a.pos : reinterpret_cast<const float*>(a.W), a.pos ? a.frames_per_clip * D * 4 : 0);
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        __builtin_amdgcn_sched_barrier(0);  // keep each sub-pass's embedding loads inside it (16 registers, not 128)
        uint32_t eoff[2];
        f32x4 pe[2][2];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int rloc = i * 16 + rr * 8;
          const uint32_t m = (uint32_t)min(mrow0 + rloc, a.M - 1);
          const uint32_t frame = a.div_tokens.div(m);
          const uint32_t tok = m - frame * (uint32_t)a.tokens;
          const uint32_t t = frame - a.div_frames.div(frame) * (uint32_t)a.frames_per_clip;
          eoff[rr] = (rloc < rows_left && tok > 0) ? ((frame * (uint32_t)(a.tokens - 1) + tok - 1) * (uint32_t)D + ecol) * 2 : 0xffffffffu;
          // no embedding (the raw export an adapter reads): add zeros, and issue no load — a register load beside
          // LDS-DMA costs a vmcnt(0) at its use, i.e. one memory round trip per sub-pass
          pe[rr][0] = pe[rr][1] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (a.pos != nullptr) {
            const uint32_t poff = (t * (uint32_t)D + ecol) * 4;
            pe[rr][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdP, poff, 0, 0));
            pe[rr][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdP, poff, 16, 0));
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<f32x4*>(parkf + (((j * 4 + eq) ^ er) << 4)) = acc[i][j];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int row = rr * 8 + drow;
          const f32x4 x0 = *reinterpret_cast<const f32x4*>(ep + row * 256 + (((2 * dc) ^ row) << 4)) + pe[rr][0];
          const f32x4 x1 = *reinterpret_cast<const f32x4*>(ep + row * 256 + (((2 * dc + 1) ^ row) << 4)) + pe[rr][1];
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o[e] = (bf16_t)x0[e];
            o[4 + e] = (bf16_t)x1[e];
          }
          store_out(__builtin_bit_cast(v4i, o), srdE, eoff[rr], a.stream_out);
        }
      }
    }
  }
  // QuickGELU on a 4-wide fragment (packed f32 arithmetic: gemm256.hip)
  auto activate = [&](f32x4 v) {
    if constexpr (EPI == DFD_EPI_BIAS_QUICKGELU) {
      float cgelu = DFD_QUICKGELU_SCALE;  // opaque + in an SGPR so that the multiply packs
      asm volatile("" : "+s"(cgelu));
      const f32x4 t = v * cgelu;
      f32x4 d;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = __builtin_amdgcn_exp2f(t[e]);
      d = d + 1.0f;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = __builtin_amdgcn_rcpf(d[e]);
      v = v * d;
    } else if constexpr (EPI == DFD_EPI_BIAS_GELU) {
      // exact-erf GELU (gelu.hpp): the same scalar function as the general kernel, so the two agree bit for bit
      v = gelu_erf4(v);
    }
    return v;
  };
  if constexpr (EPI == DFD_EPI_RESIDUAL_POS) {
    // C(bf16) = residual + dropout(acc) + pos[(row / rows_per_frame) % T], rounded ONCE (the adapter's second Linear,
    // reference models.py:795-875, :930-940; gemm256.hip has the one-workgroup-per-tile form of the same arithmetic).
    // RB sub-passes of 16 rows parked as f32 (4 KB); the drain reads the residual row segment and the positional
    // embedding (requested at the top of the sub-pass), adds and rounds; 2 stores of 8 rows x 128 B per sub-pass.
    unsigned char* const parkf = ep + er * 256;  // unit (j*4 + eq) ^ er of a 256-byte row
    const uint32_t cbase = (uint32_t)((mrow0 * a.ldc + nb + dc * 8) * 2);
    // The residual and the embedding of sub-pass i + 1 are requested before sub-pass i is drained (one sub-pass of
    // loads always in flight: with each load waited for where it is issued the epilogue is a chain of 2 RB memory
    // round trips, 29 us per tile).  Inline-asm loads, counted by hand like the K loop's: queue at the wait of sub-pass
    // i = [loads i][2 stores of i-1][6 loads of i+1].
    const v4i srdRw = a.residual ? words(reinterpret_cast<const float*>(a.residual), (int)(uint32_t)(a.M * a.ldc * 2))
                                 : words(reinterpret_cast<const float*>(a.C), (int)(uint32_t)(a.M * a.ldc * 2));
    const v4i srdQw = words(a.pos ? a.pos : reinterpret_cast<const float*>(a.W), a.pos ? a.frames_per_clip * a.N * 4 : 0);
    f32x4 pq[2][2][2];
    v4i oq[2][2];
    uint32_t offq[2][2], gq[2][2];
    auto request = [&](int i, int b) {
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int rloc = i * 16 + rr * 8;
        const uint32_t m = (uint32_t)min(mrow0 + rloc, a.M - 1);
        const uint32_t frame = a.div_tokens.div(m);  // rows per frame = tokens - 1 (the export has no CLS row)
        const uint32_t t = frame - a.div_frames.div(frame) * (uint32_t)a.frames_per_clip;
        offq[b][rr] = rloc < rows_left ? cbase + (uint32_t)rloc * (uint32_t)(a.ldc * 2) : 0xffffffffu;
        gq[b][rr] = m * (uint32_t)(a.N >> 3) + (uint32_t)((nb + dc * 8) >> 3);  // dropout group (the launcher checks M * N / 8 < 2^32)
        const uint32_t poff = a.pos ? (t * (uint32_t)a.N + (uint32_t)(nb + dc * 8)) * 4 : 0xffffffffu;  // no embedding: out of range reads 0
        asm volatile(
            "s_nop 4\n\t"
            "buffer_load_dwordx4 %0, %3, %5, 0 offen\n\t"
            "buffer_load_dwordx4 %1, %3, %5, 0 offen offset:16\n\t"
            "buffer_load_dwordx4 %2, %4, %6, 0 offen"
            : "=&v"(pq[b][rr][0]), "=&v"(pq[b][rr][1]), "=&v"(oq[b][rr])
            : "v"(poff), "v"(offq[b][rr]), "s"(srdQw), "s"(srdRw)
            : "memory");
      }
    };
    request(0, 0);
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      __builtin_amdgcn_sched_barrier(0);
      const int b = i & 1;
      if (i + 1 < RB) request(i + 1, b ^ 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(parkf + (((j * 4 + eq) ^ er) << 4)) = acc[i][j];
      if (i == 0) wait_vm<6>();
      else if (i + 1 < RB) wait_vm<8>();
      else wait_vm<2>();
      asm volatile("" : "+v"(pq[b][0][0]), "+v"(pq[b][0][1]), "+v"(oq[b][0]), "+v"(pq[b][1][0]), "+v"(pq[b][1][1]), "+v"(oq[b][1]));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int row = rr * 8 + drow;
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(ep + row * 256 + (((2 * dc) ^ row) << 4));
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(ep + row * 256 + (((2 * dc + 1) ^ row) << 4));
        float dv[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          dv[e] = x0[e];
          dv[4 + e] = x1[e];
        }
        // the adapter's last nn.Dropout, before the residual add: element index row * N + column (a multiple of 8)
        dfd_drop_eight(a.drop, (uint64_t)gq[b][rr] << 3, dv);
        const bf16x8 ob = __builtin_bit_cast(bf16x8, oq[b][rr]);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = (bf16_t)((float)ob[e] + dv[e] + pq[b][rr][0][e]);
          o[4 + e] = (bf16_t)((float)ob[4 + e] + dv[4 + e] + pq[b][rr][1][e]);
        }
        store_out(__builtin_bit_cast(v4i, o), srdC, offq[b][rr], a.stream_out);
      }
    }
  } else if constexpr (CF8) {
    // C as e4m3 of value * out_inv_scale: 4 passes of 32 rows x 64 B parked (2 KB); 8 wave-stores of 16 rows x 64 B
    stores = RB;
    const int srow = le >> 2, sc = le & 3;  // drain: row srow of a 16-row group, 16-byte chunk sc
    unsigned char* const park8 = ep + er * 64 + eq * 4;  // + ii*1024, chunk j at position j ^ ((row >> 1) & 3)
    const int psw = (er >> 1) & 3;
    const unsigned char* const dsrc8 = ep + srow * 64 + ((sc ^ ((srow >> 1) & 3)) << 4);  // + rr*1024
    const int64_t m8 = (int64_t)cur.m0 + wr * WROWS + srow;
    const int rows_left8 = (int)min((int64_t)0x7fffffff, a.M - m8);
    const uint32_t cbase8 = (uint32_t)(m8 * a.ldc + nb + sc * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = 2 * q + ii;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f32x4 v = activate(acc[i][j]) * a.out_inv_scale;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = __builtin_fminf(__builtin_fmaxf(v[e], -448.0f), 448.0f);  // e4m3 saturates at +-448
          unsigned pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0u, false);
          pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], pk, true);
          *reinterpret_cast<unsigned*>(park8 + ii * 1024 + ((j ^ psw) << 4)) = pk;
        }
      }
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const v4i d = *reinterpret_cast<const v4i*>(dsrc8 + rr * 1024);
        const int rloc = q * 32 + rr * 16;
        const uint32_t off = rloc < rows_left8 ? cbase8 + (uint32_t)rloc * (uint32_t)a.ldc : 0xffffffffu;
        store_out(d, srdC, off, a.stream_out);
      }
    }
  } else if (BLK && a.c_blocked) {
    // C fragment-blocked: the launcher permuted the output channels so that acc[i][0..3] of lane (er, eq) are channels
    // 16 eq .. + 15 of row 16 i + er of this wave's 64; acc[i][2s], acc[i][2s + 1] are the 16-byte piece (s, er, eq) of
    // unit (row group i, K tile nb / 64).  2 RB wave-stores of 1 KB of contiguous memory each: the count of the staged
    // form, so every counted wait keeps its number.  No LDS write, no LDS read, no staging wait.
    const int row0 = wr * WROWS + er;  // this lane's first row inside the tile (m0 is a multiple of 16)
    const int rows_left_b = (int)min((int64_t)0x7fffffff, a.M - ((int64_t)cur.m0 + row0));
    const uint32_t ldc2 = (uint32_t)(a.ldc * 2);
    const uint32_t cbase = dfd_blk_row((uint32_t)cur.m0 + (uint32_t)row0, ldc2) + (uint32_t)(nb >> 6) * DFD_BLK_UNIT + (uint32_t)eq * 16u;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const f32x4 v0 = activate(acc[i][2 * s]), v1 = activate(acc[i][2 * s + 1]);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = (bf16_t)v0[e];
          o[4 + e] = (bf16_t)v1[e];
        }
        const uint32_t off = i * 16 < rows_left_b ? cbase + (uint32_t)i * (ldc2 * 16u) + (uint32_t)s * 1024u : 0xffffffffu;  // rows past M: dropped
        store_out(__builtin_bit_cast(v4i, o), srdC, off, a.stream_out);
      }
    }
  } else {
    // C itself: 4 passes of 32 rows parked as bf16 (4 KB); 16 wave-stores of 8 rows x 128 B
    unsigned char* const park = ep + er * 128 + ((eq ^ ((er & 7) << 1)) << 3);  // + ii*2048, ^ (j << 5)
    const unsigned char* const dsrc = ep + drow * 128 + ((dc ^ drow) << 4);     // + rr*1024
    const uint32_t cbase = (uint32_t)((mrow0 * a.ldc + nb + dc * 8) * 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = 2 * q + ii;
        if (i >= RB) continue;  // 224-row tiles: the last pass holds 16 rows
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 v = activate(acc[i][j]);
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (bf16_t)v[e];
          // row ii*16 + er, 8-byte unit (j*4 + eq) ^ ((row & 7) << 1)
          // (the XOR is done on the LDS byte address and cast back to an LDS pointer: through a generic pointer the
          // compiler loses the address space and emits flat_store, which also counts in vmcnt)
          typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
          *reinterpret_cast<lds_bf16x4*>(((uint32_t)(uintptr_t)(lds_ptr_t)(park + ii * 2048)) ^ (uint32_t)(j << 5)) = o;
        }
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        if (q * 32 + rr * 8 >= WROWS) continue;
        const v4i d = *reinterpret_cast<const v4i*>(dsrc + rr * 1024);
        const int rloc = q * 32 + rr * 8;  // row of the store relative to this lane's first row
        uint32_t off = rloc < rows_left ? cbase + (uint32_t)rloc * (uint32_t)(a.ldc * 2) : 0xffffffffu;  // out of range: dropped
        store_out(d, srdC, off, a.stream_out);
      }
    }
  }
  return stores;
}


// ---- host side: the planned launch of kernel family L (Gemm256p / Gemm256e: `kernel`, `name`, and `run`, which launches
// one instantiation).  Nothing is decided here: the plan (gemm_plan.hpp) names the epilogue and the tile height, and a
// family instantiates exactly the forms gemm_serves lists for it.
template <class L>
int launch_persistent(const GemmPlan& p, GemmArgs& a, bool f8, bool cf8, hipStream_t st) {
  if (p.epilogue == DFD_EPI_QKV_EXPORT || p.epilogue == DFD_EPI_RESIDUAL_POS) {
    // row -> (frame, token), frame -> frame % T; RESIDUAL_POS rows have no CLS row
    a.div_tokens = FastDiv::make((uint32_t)(p.epilogue == DFD_EPI_RESIDUAL_POS ? a.tokens - 1 : a.tokens));
    a.div_frames = FastDiv::make((uint32_t)(a.frames_per_clip > 0 ? a.frames_per_clip : 1));
  }
  auto go = [&](auto epi_c) -> int {
    constexpr int EPI = decltype(epi_c)::value;
    if (f8) {  // e4m3 operands: 256-row tiles; C bf16, or e4m3 where no row maps to a frame
      if constexpr (gemm_serves(L::kernel, EPI, true)) {
        if constexpr (EPI != DFD_EPI_QKV_EXPORT) {
          if (cf8) return L::template run<EPI, 8, true, true>(p, st, a);
        }
        return L::template run<EPI, 8, true, false>(p, st, a);
      }
    } else if constexpr (gemm_serves(L::kernel, EPI, false)) {
      if (p.tiles.rows == 224) return L::template run<EPI, 7, false, false>(p, st, a);
      if constexpr (EPI != DFD_EPI_RESIDUAL_POS) return L::template run<EPI, 8, false, false>(p, st, a);  // (that epilogue only exists for 224-row tiles)
    }
    return DFD_ERR_INVALID_ARG;  // not reached: the plan names no form a family lacks
  };
  switch (p.epilogue) {
    case DFD_EPI_BIAS:
      return go(std::integral_constant<int, DFD_EPI_BIAS>{});
    case DFD_EPI_BIAS_QUICKGELU:
      return go(std::integral_constant<int, DFD_EPI_BIAS_QUICKGELU>{});
    case DFD_EPI_BIAS_GELU:
      return go(std::integral_constant<int, DFD_EPI_BIAS_GELU>{});
    case DFD_EPI_QKV_EXPORT:
      return go(std::integral_constant<int, DFD_EPI_QKV_EXPORT>{});
    case DFD_EPI_RESIDUAL_POS:
      return go(std::integral_constant<int, DFD_EPI_RESIDUAL_POS>{});
    default:
      return DFD_ERR_INVALID_ARG;
  }
}

}  // namespace
