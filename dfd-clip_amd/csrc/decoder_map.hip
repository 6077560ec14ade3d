// Decoder attention map (include/dfdclip_explain.h): the per-key weight ½·(w_softmax + w_coda) that
// decoder_attn_partial_kernel (decoder.hip) folds into its accumulators and never stores.
//
// dfd_decoder_attn_map — one pass over K.  Lane mapping, row loads and the three reductions of a row are the forward's
//   (key_trip of decoder_common.hpp, without the value rows: the sums carry the forward's bits); the softmax weight
//   is normalised with the (max, sumexp) the forward's combine kernel wrote, so no second pass and no reduction across
//   workgroups are needed.  A workgroup owns `per` consecutive keys of one clip for all heads; the lane that finishes a row
//   puts its two weights into LDS ([2][heads][per]), and after one barrier the workgroup writes each head's run of `per`
//   contiguous floats with 16-byte stores (dword stores only before the first and after the last 16-byte boundary of the
//   run: S need not be a multiple of 4, so runs start at any dword).
// dfd_decoder_attn_map_frames (include/dfdclip_kvtable.h) — the same kernel with TAB: K is a frame store read through the
//   slot table that dfd_decoder_attn_fwd_frames read it through.
#include "decoder_common.hpp"
#include "../../include/dfdclip_explain.h"
#include "../../include/dfdclip_kvtable.h"

namespace {

// dst[h*S + j] = val(h, j) for h < heads, j < n: slot 0 of a head is the piece before the first 16-byte boundary, slot
// c >= 1 the c-th aligned piece; a piece that is not whole goes out dword by dword
template <typename F>
__device__ __forceinline__ void store_runs(float* dst0, int64_t S, int heads, int n, int slots, F val) {
  for (int idx = threadIdx.x; idx < heads * slots; idx += blockDim.x) {
    const int h = idx / slots, c = idx - h * slots;
    float* dst = dst0 + (int64_t)h * S;
    const int lead = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2);
    const int j0 = lead + 4 * (c - 1);
    if (c >= 1 && j0 + 4 <= n) {
      *reinterpret_cast<f32x4*>(dst + j0) = f32x4{val(h, j0), val(h, j0 + 1), val(h, j0 + 2), val(h, j0 + 3)};
    } else {
      const int lo = c == 0 ? 0 : j0, hi = min(n, c == 0 ? lead : j0 + 4);
      for (int j = lo; j < hi; ++j) dst[j] = val(h, j);
    }
  }
}

template <typename T, int MAXT, bool POS, bool TAB>
__global__ __launch_bounds__(MAXT) void decoder_attn_map_kernel(const float* __restrict__ q, const T* __restrict__ k,
                                                               const uint8_t* __restrict__ frame_mask,
                                                               const float* __restrict__ stats, const float* __restrict__ ext_w,
                                                               float* __restrict__ aff, float* __restrict__ branches,
                                                               int64_t branch_stride, int per, int T_frames, int patches,
                                                               int heads, int R, KvLayout lay, FastDiv div_patches,
                                                               const int32_t* __restrict__ frame_table, int store_frames) {
  extern __shared__ float wl[];  // [2][heads][per] branch weights, then (POS) the positional embedding of this block's frames, then (TAB) T slots
  const HeadLanes ln(heads);
  const int hd = ln.hd;
  const int b = blockIdx.y;
  const int S = T_frames * patches;
  const int D = heads * HD;
  const int s_begin = blockIdx.x * per;  // < S: the grid has ceil(S / per) blocks per clip
  const int s_end = min(S, s_begin + per);
  float* const posl = wl + (size_t)2 * heads * per;
  const int* const ftab = stage_slots<TAB, POS>(posl, frame_table, store_frames, b, T_frames, s_begin, s_end, S, D, div_patches);
  const int f0 = stage_pos<POS>(posl, lay.pos, s_begin, s_end, S, D, div_patches);

  float qs[8], qc[8];
  load_query(q, b, heads, ln, 0.125f, qs, qc);
  float mx = 0.f, l = 1.f;
  if (ext_w == nullptr) {
    mx = stats[((int64_t)b * heads + hd) * 2 + 0];
    l = stats[((int64_t)b * heads + hd) * 2 + 1];
  }

  const T* kb = ln.channels(k + (TAB ? 0 : (int64_t)b * T_frames * lay.frame_stride));
  const KeySpan sp{s_end, S, D, f0, patches, R, lay, div_patches, frame_mask + (int64_t)b * T_frames, ln.channels(posl), ftab};
  float* const ws = wl + (size_t)hd * per;                  // softmax branch of my head
  float* const wc = wl + (size_t)(heads + hd) * per;        // CoDA branch
  for (int s0 = s_begin + ln.rs; s0 < s_end; s0 += UN * R) {
    Raw8<T> no_v[1];
    int po[UN];
    const KeyRow me = key_trip<T, POS, false, false, TAB>(sp, ln, qs, qc, kb, kb, s0, no_v, po);
    if (me.s < s_end) {
      float p;
      if (ext_w != nullptr) p = me.ok ? ext_w[((int64_t)b * heads + hd) * S + me.s] : 0.f;
      else p = me.ok ? __expf(me.ds - mx) / l : 0.f;
      ws[me.s - s_begin] = p;
      wc[me.s - s_begin] = me.ok ? coda_weight(me.dc, me.l1) : 0.f;
    }
  }
  __syncthreads();
  const int n = s_end - s_begin;
  const int slots = (per >> 2) + 1;  // per % 4 == 0
  const int64_t row0 = (int64_t)b * heads * S + s_begin;
  const float* wlc = wl;
  const int hp = heads * per;
  store_runs(aff + row0, S, heads, n, slots, [=](int h, int j) { return 0.5f * (wlc[h * per + j] + wlc[hp + h * per + j]); });
  if (branches != nullptr) {
    store_runs(branches + row0, S, heads, n, slots, [=](int h, int j) { return wlc[h * per + j]; });
    store_runs(branches + branch_stride + row0, S, heads, n, slots, [=](int h, int j) { return wlc[hp + h * per + j]; });
  }
}

}  // namespace

namespace {

// dfd_decoder_attn_map (frame_table == nullptr) and dfd_decoder_attn_map_frames: one check, one plan, the TAB flag apart
int decoder_attn_map(const char* who, const float* q, const void* k, int kv_dtype, const dfd_kv_layout_t* layout,
                     const uint8_t* frame_mask, const float* stats, const float* ext_weights, float* aff, float* branches, int B,
                     int T, int patches, int heads, int d, const int32_t* frame_table, int store_frames, void* stream) {
  const bool tab = frame_table != nullptr;
  if (int rc = check_decoder_attn(who, q && k && aff && frame_mask && (stats || ext_weights), {k, q}, kv_dtype, layout, B, T, patches,
                                  heads, d))
    return rc;
  DFD_REQUIRE((int64_t)T * patches < (1ll << 30), "%s: bad shape", who);
  DFD_REQUIRE((reinterpret_cast<uintptr_t>(aff) & 3) == 0 && (reinterpret_cast<uintptr_t>(branches) & 3) == 0,
              "%s: aff and branches must be 4-byte aligned", who);
  if (B == 0) return DFD_OK;
  const KvLayout lay = dfd_kv_layout(layout, patches, heads * HD);
  const FastDiv divp = FastDiv::make((uint32_t)patches);
  const AttnBlock blk = decoder_attn_block(heads);
  const int R = blk.R;
  const int S = T * patches;
  // keys per workgroup: up to 4 trips of 8R rows, fewer while the LDS (weights + staged positional rows) exceeds 64 KB
  // or the clip has no more rows
  int trips = 4;
  size_t lds = 0;
  int per = 0;
  for (;; --trips) {
    per = UN * R * trips;
    const int span = lay.pos ? (per + patches - 2) / patches + 1 : 0;  // frames a block's rows can touch
    lds = (size_t)2 * heads * per * sizeof(float) + (size_t)(span < T ? span : T) * heads * HD * sizeof(float) +
          (tab ? (size_t)T * sizeof(int) : 0);  // the clip's staged slots
    if (trips == 1 || (lds <= 64 * 1024 && UN * R * (trips - 1) < S)) break;
  }
  DFD_REQUIRE(lds <= 160 * 1024, "%s: %zu B of LDS", who, lds);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t branch_stride = (int64_t)B * heads * S;
  const Launch launch{dim3((S + per - 1) / per, B), dim3(blk.threads), lds, st};
  // the map's K loads are plain (no NT form)
  return decoder_attn_dispatch(kv_dtype, blk.threads, lay.pos != nullptr, false, [&](auto kt, auto mt, auto ps, auto) {
    using KT = typename decltype(kt)::type;
    return pick(tab, [&](auto tb) {
      return launch_kernel(who, decoder_attn_map_kernel<KT, decltype(mt)::value, decltype(ps)::value, decltype(tb)::value>, launch, q, k,
                           frame_mask, stats, ext_weights, aff, branches, branch_stride, per, T, patches, heads, R, lay, divp,
                           frame_table, store_frames);
    });
  });
}

}  // namespace

extern "C" int dfd_decoder_attn_map(const float* q, const void* k, int kv_dtype, const dfd_kv_layout_t* layout,
                                    const uint8_t* frame_mask, const float* stats, const float* ext_weights, float* aff,
                                    float* branches, int B, int T, int patches, int heads, int d, void* stream) {
  return decoder_attn_map("dfd_decoder_attn_map", q, k, kv_dtype, layout, frame_mask, stats, ext_weights, aff, branches, B, T, patches,
                          heads, d, nullptr, 0, stream);
}

extern "C" int dfd_decoder_attn_map_frames(const float* q, const void* k, int kv_dtype, const dfd_kv_layout_t* layout,
                                           const uint8_t* frame_mask, const float* stats, const float* ext_weights, float* aff,
                                           float* branches, int B, int T, int patches, int heads, int d, const int32_t* frame_table,
                                           int store_frames, void* stream) {
  if (int rc = check_frame_table("dfd_decoder_attn_map_frames", frame_table, store_frames)) return rc;
  return decoder_attn_map("dfd_decoder_attn_map_frames", q, k, kv_dtype, layout, frame_mask, stats, ext_weights, aff, branches, B, T,
                          patches, heads, d, frame_table, store_frames, stream);
}
