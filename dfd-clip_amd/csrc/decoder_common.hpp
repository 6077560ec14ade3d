// The decoder's single-query attention, written once for its forward (decoder.hip), backward (decoder_bwd.hip) and
// attention-map (decoder_map.hip) kernels.  Device: 8-element row pieces (one lane's share of a 64-wide head), the exchanges
// inside an 8-lane head group, tanh, and the key-row front: the lane mapping of a workgroup, the query load, the staging
// of the positional embedding, and the eight-row trip that leaves each lane with the three sums of its own key row.  Host:
// the argument check of the five entry points, the block-size rule, the launch helper and the dispatch from (key type,
// block size, POS, NT) to an instantiation.  A new K/V addressing mode is an edit of kv_row_offset / key_trip, of
// check_decoder_attn and of the backward's walk over its one frame.  TAB is one: the forward and the map read the frames
// of a clip out of a frame store through a slot table (include/dfdclip_kvtable.h); the backward does not.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "stream_policy.hpp"

// out[b, h, s] = scale * Σ_c a[b, h, c] · X[b, s, h*64 + c], `fill` on the keys of padded frames when a mask is given
// (decoder.hip; the attn_mode entry points of decoder.hip and decoder_bwd.hip score their keys with it)
int dfd_decoder_rowdot(const float* a, int a_stride, const void* X, int kv_dtype, const dfd_kv_layout_t* layout,
                       const uint8_t* frame_mask, float* out, float scale, float fill, int B, int T, int patches, int heads,
                       hipStream_t st);

namespace {

constexpr int HD = 64;            // channels of a head
constexpr int PART = 2 + 2 * HD;  // floats per (clip, split, head) of the forward's workspace: m, l, acc_s[64], acc_c[64]
constexpr int UN = 8;             // key rows per trip of the forward and the map: one per lane of the 8-lane head group

template <typename T> struct Ld8;
template <> struct Ld8<float> {
  static __device__ __forceinline__ void load(const float* p, float* o) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = a[e]; o[4 + e] = b[e]; }
  }
};
template <> struct Ld8<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* o) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (float)a[e];
  }
};

__device__ __forceinline__ float group8_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

__device__ __forceinline__ float group8_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64));
  v = fmaxf(v, __shfl_xor(v, 2, 64));
  v = fmaxf(v, __shfl_xor(v, 4, 64));
  return v;
}
// x[u] = this lane's partial sum for row u (u = 0..7); returns the 8-lane group's total for row `sub` (the lane's
// index in its group): 7 exchanges instead of the 24 of eight butterflies
__device__ __forceinline__ float group8_reduce_scatter(const float (&x)[8], int sub) {
  float y[4], z[2];
  const bool h4 = (sub & 4) != 0, h2 = (sub & 2) != 0, h1 = (sub & 1) != 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = (h4 ? x[i + 4] : x[i]) + __shfl_xor(h4 ? x[i] : x[i + 4], 4, 64);
#pragma unroll
  for (int i = 0; i < 2; ++i) z[i] = (h2 ? y[i + 2] : y[i]) + __shfl_xor(h2 ? y[i] : y[i + 2], 2, 64);
  return (h1 ? z[1] : z[0]) + __shfl_xor(h1 ? z[0] : z[1], 1, 64);
}

// four rows per trip: x[u] = this lane's partial sum for row u (u = 0..3); returns the group's total for row
// `sub & 3` (lanes j and j + 4 finish the same row): 7 exchanges instead of the 12 of four butterflies
__device__ __forceinline__ float group8_reduce_scatter4(const float (&x)[4], int sub) {
  float y[4], z[2];
  const bool h2 = (sub & 2) != 0, h1 = (sub & 1) != 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = x[i] + __shfl_xor(x[i], 4, 64);
#pragma unroll
  for (int i = 0; i < 2; ++i) z[i] = (h2 ? y[i + 2] : y[i]) + __shfl_xor(h2 ? y[i] : y[i + 2], 2, 64);
  return (h1 ? z[1] : z[0]) + __shfl_xor(h1 ? z[0] : z[1], 1, 64);
}

// eight consecutive elements as loaded (bf16: 16 bytes, f32: 32 bytes), converted where they are used; NT: the
// non-temporal form, for the K / V rows a kernel reads once (DFD_STREAM_DECODER_KV)
template <typename T> struct Raw8;
template <> struct Raw8<float> {
  f32x4 a, b;
  template <bool NT = false> __device__ __forceinline__ void load(const float* p) { a = stream_load16<NT>(p); b = stream_load16<NT>(p + 4); }
  __device__ __forceinline__ float get(int e) const { return e < 4 ? a[e] : b[e - 4]; }
};
template <> struct Raw8<bf16_t> {
  bf16x8 a;
  template <bool NT = false> __device__ __forceinline__ void load(const bf16_t* p) { a = __builtin_bit_cast(bf16x8, stream_load16<NT>(p)); }
  __device__ __forceinline__ float get(int e) const { return (float)a[e]; }
};

__device__ __forceinline__ float fast_tanh(float x) {
  // tanh(x) = 1 - 2/(exp(2x)+1); exact limits at +-inf, abs error ~1e-7 around 0
  const float e = __expf(2.0f * x);
  return 1.0f - 2.0f / (e + 1.0f);
}

// One channel of a key row folded into the lane's three partial sums against the clip's query: ds += q_s·k/√d (qs is
// pre-scaled), dc += q_c·k/√d, l1 += |q_c − k|, d = 64.  Shared by the forward (decoder.hip) and the attention map
// (decoder_map.hip), so that both form the same bits.
__device__ __forceinline__ void key_channel(float kk, float qs, float qc, float& ds, float& dc, float& l1) {
  ds = fmaf(qs, kk, ds);
  dc = fmaf(qc * 0.125f, kk, dc);
  l1 += fabsf(qc - kk);
}

// CoDA weight of a key from its reduced sums: tanh(q_c·k/√d) · 2·sigmoid(−‖q_c − k‖₁/√d), d = 64; the backward needs
// the two factors apart
__device__ __forceinline__ float coda_gate(float l1) { return 2.0f / (1.0f + __expf(l1 * 0.125f)); }
__device__ __forceinline__ float coda_weight(float dc, float l1) {
  const float gate = coda_gate(l1);
  return fast_tanh(dc) * gate;
}

// ---- the key-row front ---------------------------------------------------------------------------------------------
// A workgroup is R row slots of heads*8 lanes: slot `rs` takes every R-th key row, lane `tr` of a slot the 8 channels
// from hd*64 + sub*8 (lane `sub` of the 8-lane group of head `hd`); `lane_base` is the group's first lane in its wave.
struct HeadLanes {
  int tpr, rs, tr, hd, sub, lane_base;
  __device__ __forceinline__ explicit HeadLanes(int heads)
      : tpr(heads * 8), rs(threadIdx.x / tpr), tr(threadIdx.x % tpr), hd(tr >> 3), sub(tr & 7), lane_base((threadIdx.x & 63) & ~7) {}
  // the lane's 8 channels of a [heads*64]-wide row
  template <typename P> __device__ __forceinline__ P* channels(P* row) const { return row + hd * HD + sub * 8; }
};

// the lane's share of clip b's two queries, q = [softmax | CoDA] per head; the forward and the map fold 1/√d into qs
__device__ __forceinline__ void load_query(const float* q, int b, int heads, const HeadLanes& ln, float scale, float (&qs)[8],
                                           float (&qc)[8]) {
  const float* qp = q + ((int64_t)b * heads + ln.hd) * (2 * HD) + ln.sub * 8;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    qs[e] = qp[e] * scale;
    qc[e] = qp[HD + e];
  }
}

// row s of a clip = patch s % patches of its frame tf = s / patches (KvLayout: dense export or the qkv activation in place).
// TAB: the frame is frame slots[tf] of a store, not frame tf of the clip (`slots`: the clip's T entries as stage_slots left
// them, clamped); the offset is then relative to the store's base, and the product is formed in 64 bits like the other.
template <bool TAB = false>
__device__ __forceinline__ int64_t kv_row_offset(int s, int patches, const KvLayout& lay, const FastDiv& div_patches, int& tf,
                                                 const int* slots = nullptr) {
  tf = (int)div_patches.div((uint32_t)s);
  int f = tf;
  if constexpr (TAB) f = slots[tf];
  return (int64_t)f * lay.frame_stride + (int64_t)(s - tf * patches) * lay.row_stride;
}

// POS: the rows [s_begin, s_end) of a workgroup lie in frames f0 .. f1 of the clip; their positional embeddings are staged
// at `posl`, behind the kernel's own LDS, once (held in registers they cost the forward half its occupancy).  A workgroup
// without rows (s_begin >= s_end) stages one frame.  Returns f0.
template <bool POS>
__device__ __forceinline__ int stage_pos(float* posl, const float* pos, int s_begin, int s_end, int S, int D,
                                         const FastDiv& div_patches) {
  const int f0 = (int)div_patches.div((uint32_t)min(s_begin, S - 1));
  if constexpr (POS) {
    const int last = max(s_end, s_begin + 1) - 1;
    const int f1 = (int)div_patches.div((uint32_t)(last < S ? last : S - 1));
    const int n4 = (f1 - f0 + 1) * (D >> 2);
    for (int i = threadIdx.x; i < n4; i += blockDim.x)
      reinterpret_cast<f32x4*>(posl)[i] = reinterpret_cast<const f32x4*>(pos + (int64_t)f0 * D)[i];
    __syncthreads();
  }
  return f0;
}

// TAB: the T slots of clip b (frame_table[b*T .. b*T + T)) are staged once per workgroup in the dynamic LDS behind the
// positional rows that stage_pos puts at `posl`, each clamped to [0, store_frames) on the way (the rule of kv_frames.hip:
// no address is formed from an entry as given).  Staged, not read per row through the cache, by the compiler's report
// (profiles/decoder_table_resources.txt): staged, every tabled instantiation has the VGPRs and the occupancy of its untabled
// twin, one ds_read_b32 per row and no further barrier with POS; read per row (a global load and a clamp in front of every
// K / V load) the forward's 512-thread bf16 forms, the ones ViT-B/16 runs, take 6 to 7 VGPRs more and the map up to 11.
// Call it BEFORE stage_pos: with POS that call's barrier covers the slots too; without POS the barrier is here.  Returns
// the staged slots (nullptr without TAB: nothing is staged or read).
template <bool TAB, bool POS>
__device__ __forceinline__ const int* stage_slots(float* posl, const int32_t* frame_table, int store_frames, int b, int T_frames,
                                                  int s_begin, int s_end, int S, int D, const FastDiv& div_patches) {
  if constexpr (!TAB) {
    return nullptr;
  } else {
    int* sl = reinterpret_cast<int*>(posl);
    if constexpr (POS) {  // behind the frames f0 .. f1 that stage_pos stages (the same two divisions)
      const int f0 = (int)div_patches.div((uint32_t)min(s_begin, S - 1));
      const int last = max(s_end, s_begin + 1) - 1;
      const int f1 = (int)div_patches.div((uint32_t)(last < S ? last : S - 1));
      sl += (f1 - f0 + 1) * D;
    }
    const int32_t* tb = frame_table + (int64_t)b * T_frames;
    for (int i = threadIdx.x; i < T_frames; i += blockDim.x) sl[i] = min(max(tb[i], 0), store_frames - 1);
    if constexpr (!POS) __syncthreads();
    return sl;
  }
}

// the keys of one clip up to s_end, as a workgroup walks them
struct KeySpan {
  int s_end, S, D, f0, patches, R;
  KvLayout lay;
  FastDiv div_patches;
  const uint8_t* mb;  // the clip's frame mask
  const float* pb;    // POS: the lane's channels of frame f0 in the staged positional embedding
  const int* slots;   // TAB: the clip's staged frame slots (stage_slots); the mask and `pb` stay indexed by the clip's frame
};
// the lane's own row of a trip: its three sums over the head, its index, and whether it is a key (in range, frame valid)
struct KeyRow {
  float ds, dc, l1;
  int s;
  bool ok;
};

// Eight rows per trip, s0 + u*R for u = 0..7, one per lane of the 8-lane head group, all loads issued before the first
// use (the loop is a latency chain otherwise).  Every lane forms its 8-channel share of the three dot products of all eight
// rows; a reduce-scatter over the group leaves lane j with the totals of row j, so the row's transcendentals (exp, tanh,
// sigmoid: the VALU bulk of these kernels) run ONCE per row instead of once per lane.  kb / vb: the lane's channels of
// the clip's first row (TAB: of the store's first row); WITH_V keeps the value rows in vr for the caller; po[u]: offset of
// row u's frame behind sp.pb.
template <typename T, bool POS, bool NT, bool WITH_V, bool TAB = false>
__device__ __forceinline__ KeyRow key_trip(const KeySpan& sp, const HeadLanes& ln, const float (&qs)[8], const float (&qc)[8],
                                           const T* kb, const T* vb, int s0, Raw8<T> (&vr)[WITH_V ? UN : 1], int (&po)[UN]) {
  Raw8<T> kr[UN];
#pragma unroll
  for (int u = 0; u < UN; ++u) {
    int tf;
    const int s = min(s0 + u * sp.R, sp.s_end - 1);  // clamp: rows past the end are loaded but not used
    const int64_t off = kv_row_offset<TAB>(s, sp.patches, sp.lay, sp.div_patches, tf, sp.slots);
    kr[u].template load<NT>(kb + off);
    if constexpr (WITH_V) vr[u].template load<NT>(vb + off);
    po[u] = (tf - sp.f0) * sp.D;
  }
  float pds[UN], pdc[UN], pl1[UN];
#pragma unroll
  for (int u = 0; u < UN; ++u) {
    float ds = 0.f, dc = 0.f, l1 = 0.f;
    [[maybe_unused]] float pe[8];
    if constexpr (POS) Ld8<float>::load(sp.pb + po[u], pe);
#pragma unroll
    for (int e = 0; e < 8; ++e) key_channel(POS ? kr[u].get(e) + pe[e] : kr[u].get(e), qs[e], qc[e], ds, dc, l1);
    pds[u] = ds;
    pdc[u] = dc;
    pl1[u] = l1;
  }
  KeyRow me;
  me.ds = group8_reduce_scatter(pds, ln.sub);
  me.dc = group8_reduce_scatter(pdc, ln.sub);
  me.l1 = group8_reduce_scatter(pl1, ln.sub);
  me.s = s0 + ln.sub * sp.R;
  me.ok = me.s < sp.s_end && sp.mb[sp.div_patches.div((uint32_t)min(me.s, sp.S - 1))] != 0;
  return me;
}

// ---- host: one argument check and one launch plan ------------------------------------------------------------------
// key rows side by side in a workgroup: at least 256 threads, whole waves
struct AttnBlock {
  int R, threads;  // threads = heads*8*R; <= 512 takes the 512-thread form of a kernel, else the 1024-thread form
};
inline AttnBlock decoder_attn_block(int heads) {
  const int tpr = heads * 8;
  int R = (256 + tpr - 1) / tpr;
  while ((tpr * R) % 64 != 0) ++R;
  return AttnBlock{R, tpr * R};
}

// What all five decoder-attention entry points refuse, in the same words: `given` is the entry point's own "no NULL among
// the required pointers", `aligned16` the pointers its kernels read with 16-byte loads.
inline int check_decoder_attn(const char* who, bool given, std::initializer_list<const void*> aligned16, int kv_dtype,
                              const dfd_kv_layout_t* l, int B, int T, int patches, int heads, int d) {
  DFD_REQUIRE(given, "%s: null pointer", who);
  DFD_REQUIRE(d == HD, "%s: head dim %d, only 64 is supported", who, d);
  DFD_REQUIRE(B >= 0 && T > 0 && patches > 0 && heads > 0 && heads * HD <= 4096, "%s: bad shape", who);  // (4096: dfd_layernorm's widest row)
  DFD_REQUIRE(decoder_attn_block(heads).threads <= 1024, "%s: heads=%d needs %d threads", who, heads, decoder_attn_block(heads).threads);
  DFD_REQUIRE(kv_dtype == DFD_F32 || kv_dtype == DFD_BF16, "%s: kv_dtype=%d", who, kv_dtype);
  for (const void* p : aligned16) DFD_REQUIRE(dfd_aligned16(p), "%s: pointers must be 16-byte aligned", who);
  if (l == nullptr) return DFD_OK;
  const int per16 = kv_dtype == DFD_F32 ? 4 : 8;
  DFD_REQUIRE(l->row_stride >= heads * HD && l->frame_stride > 0 && l->row_stride % per16 == 0 && l->frame_stride % per16 == 0,
              "%s: key/value layout: row stride %lld, frame stride %lld (elements; rows must stay 16-byte aligned)", who,
              (long long)l->row_stride, (long long)l->frame_stride);
  DFD_REQUIRE(!l->pos || dfd_aligned16(l->pos), "%s: the positional embedding must be 16-byte aligned", who);
  return DFD_OK;
}

// What the two frame-table entry points (include/dfdclip_kvtable.h) refuse on top of check_decoder_attn.
inline int check_frame_table(const char* who, const int32_t* frame_table, int store_frames) {
  DFD_REQUIRE(frame_table != nullptr, "%s: null frame table", who);
  DFD_REQUIRE(store_frames > 0, "%s: store_frames=%d: the store needs at least one frame", who, store_frames);
  return DFD_OK;
}

// Raise the kernel's dynamic-LDS limit where static + dynamic LDS pass the 64 KiB a launch gets unasked, launch, report.
struct Launch {
  dim3 grid, block;
  size_t lds;
  hipStream_t st;
  size_t static_lds = 0;
};
template <typename... P, typename... A>
int launch_kernel(const char* what, void (*kernel)(P...), const Launch& l, A... args) {
  if (l.lds + l.static_lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds);
  hipLaunchKernelGGL(kernel, l.grid, l.block, l.lds, l.st, static_cast<P>(args)...);
  DFD_CHECK_LAUNCH(what);
  return DFD_OK;
}

// f(std::true_type{}) or f(std::false_type{}): a run-time flag becomes a template argument
template <typename F> int pick(bool c, F&& f) { return c ? f(std::true_type{}) : f(std::false_type{}); }

// (kv_dtype, block size, POS, NT) -> f(key type tag, MAXT, POS, NT), every argument a compile-time constant; a kernel
// without one of the parameters ignores its tag and passes false
template <typename T> struct TypeTag { using type = T; };
template <typename F> int decoder_attn_dispatch(int kv_dtype, int threads, bool pos, bool nt, F&& f) {
  return pick(kv_dtype == DFD_F32, [&](auto f32) {
    return pick(threads <= 512, [&](auto small) {
      return pick(pos, [&](auto ps) {
        return pick(nt, [&](auto ntc) {
          return f(TypeTag<std::conditional_t<decltype(f32)::value, float, bf16_t>>{},
                   std::integral_constant<int, decltype(small)::value ? 512 : 1024>{}, ps, ntc);
        });
      });
    });
  });
}

}  // namespace
