// Decoder attention map (include/dfdclip_explain.h): the per-key weight ½·(w_softmax + w_coda) that
// decoder_attn_partial_kernel (decoder.hip) folds into its accumulators and never stores.
//
// dfd_decoder_attn_map — one pass over K.  Lane mapping, row loads and the three reductions of a row are the forward's
//   (key_channel + group8_reduce_scatter of decoder_common.hpp: the sums carry the forward's bits); the softmax weight
//   is normalised with the (max, sumexp) the forward's combine kernel wrote, so no second pass and no reduction across
//   workgroups are needed.  A workgroup owns `per` consecutive keys of one clip for all heads; the lane that finishes a row
//   puts its two weights into LDS ([2][heads][per]), and after one barrier the workgroup writes each head's run of `per`
//   contiguous floats with 16-byte stores (dword stores only before the first and after the last 16-byte boundary of the
//   run: S need not be a multiple of 4, so runs start at any dword).
#include "decoder_common.hpp"
#include "../../include/dfdclip_explain.h"

namespace {

constexpr int HD = 64;
constexpr int UN = 8;  // rows per trip, one per lane of the 8-lane head group (as the forward)

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

template <typename T, int MAXT, bool POS>
__global__ __launch_bounds__(MAXT) void decoder_attn_map_kernel(const float* __restrict__ q, const T* __restrict__ k,
                                                               const uint8_t* __restrict__ frame_mask,
                                                               const float* __restrict__ stats, const float* __restrict__ ext_w,
                                                               float* __restrict__ aff, float* __restrict__ branches,
                                                               int64_t branch_stride, int per, int T_frames, int patches,
                                                               int heads, int R, KvLayout lay, FastDiv div_patches) {
  extern __shared__ float wl[];  // [2][heads][per] branch weights, then (POS) the positional embedding of this block's frames
  const int tpr = heads * 8;
  const int b = blockIdx.y;
  const int rs = threadIdx.x / tpr, tr = threadIdx.x % tpr;
  const int hd = tr >> 3, sub = tr & 7;
  const int S = T_frames * patches;
  const int D = heads * HD;
  const int s_begin = blockIdx.x * per;  // < S: the grid has ceil(S / per) blocks per clip
  const int s_end = min(S, s_begin + per);
  [[maybe_unused]] float* const posl = wl + (size_t)2 * heads * per;
  [[maybe_unused]] const int f0 = (int)div_patches.div((uint32_t)s_begin);
  if constexpr (POS) {
    const int f1 = (int)div_patches.div((uint32_t)(s_end - 1));
    const int n4 = (f1 - f0 + 1) * (D >> 2);
    for (int i = threadIdx.x; i < n4; i += blockDim.x)
      reinterpret_cast<f32x4*>(posl)[i] = reinterpret_cast<const f32x4*>(lay.pos + (int64_t)f0 * D)[i];
    __syncthreads();
  }

  float qs[8], qc[8];
  {
    const float* qp = q + ((int64_t)b * heads + hd) * (2 * HD) + sub * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      qs[e] = qp[e] * 0.125f;
      qc[e] = qp[HD + e];
    }
  }
  float mx = 0.f, l = 1.f;
  if (ext_w == nullptr) {
    mx = stats[((int64_t)b * heads + hd) * 2 + 0];
    l = stats[((int64_t)b * heads + hd) * 2 + 1];
  }

  const T* kb = k + (int64_t)b * T_frames * lay.frame_stride + hd * HD + sub * 8;
  [[maybe_unused]] const float* const pb = posl + hd * HD + sub * 8;
  const uint8_t* mb = frame_mask + (int64_t)b * T_frames;
  float* const ws = wl + (size_t)hd * per;                  // softmax branch of my head
  float* const wc = wl + (size_t)(heads + hd) * per;        // CoDA branch
  for (int s0 = s_begin + rs; s0 < s_end; s0 += UN * R) {
    Raw8<T> kr[UN];
    [[maybe_unused]] int po[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int s = min(s0 + u * R, s_end - 1);  // clamp: rows past the end are loaded but not used
      const int tf = (int)div_patches.div((uint32_t)s);
      kr[u].load(kb + (int64_t)tf * lay.frame_stride + (int64_t)(s - tf * patches) * lay.row_stride);
      po[u] = (tf - f0) * D;
    }
    float pds[UN], pdc[UN], pl1[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      float ds = 0.f, dc = 0.f, l1 = 0.f;
      [[maybe_unused]] float pe[8];
      if constexpr (POS) Ld8<float>::load(pb + po[u], pe);
#pragma unroll
      for (int e = 0; e < 8; ++e) key_channel(POS ? kr[u].get(e) + pe[e] : kr[u].get(e), qs[e], qc[e], ds, dc, l1);
      pds[u] = ds;
      pdc[u] = dc;
      pl1[u] = l1;
    }
    const float ds = group8_reduce_scatter(pds, sub), dc = group8_reduce_scatter(pdc, sub), l1 = group8_reduce_scatter(pl1, sub);
    // my row of this trip
    const int s_me = s0 + sub * R;
    if (s_me < s_end) {
      const bool ok = mb[div_patches.div((uint32_t)s_me)] != 0;
      float p;
      if (ext_w != nullptr) p = ok ? ext_w[((int64_t)b * heads + hd) * S + s_me] : 0.f;
      else p = ok ? __expf(ds - mx) / l : 0.f;
      ws[s_me - s_begin] = p;
      wc[s_me - s_begin] = ok ? coda_weight(dc, l1) : 0.f;
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

int map_rows_per_block(int heads) {  // as the forward's: >= 256 threads, whole waves
  const int tpr = heads * 8;
  int R = (256 + tpr - 1) / tpr;
  while ((tpr * R) % 64 != 0) ++R;
  return R;
}

}  // namespace

extern "C" int dfd_decoder_attn_map(const float* q, const void* k, int kv_dtype, const dfd_kv_layout_t* layout,
                                    const uint8_t* frame_mask, const float* stats, const float* ext_weights, float* aff,
                                    float* branches, int B, int T, int patches, int heads, int d, void* stream) {
  DFD_REQUIRE(q && k && aff && frame_mask && (stats || ext_weights), "dfd_decoder_attn_map: null pointer");
  DFD_REQUIRE(d == HD, "dfd_decoder_attn_map: head dim %d, only 64 is supported", d);
  DFD_REQUIRE(B >= 0 && T > 0 && patches > 0 && heads > 0 && heads * HD <= 1024 && (int64_t)T * patches < (1ll << 30),
              "dfd_decoder_attn_map: bad shape");
  DFD_REQUIRE(kv_dtype == DFD_F32 || kv_dtype == DFD_BF16, "dfd_decoder_attn_map: kv_dtype=%d", kv_dtype);
  DFD_REQUIRE(dfd_aligned16(k) && dfd_aligned16(q), "dfd_decoder_attn_map: q and k must be 16-byte aligned");
  DFD_REQUIRE((reinterpret_cast<uintptr_t>(aff) & 3) == 0 && (reinterpret_cast<uintptr_t>(branches) & 3) == 0,
              "dfd_decoder_attn_map: aff and branches must be 4-byte aligned");
  if (layout != nullptr) {
    const int per16 = kv_dtype == DFD_F32 ? 4 : 8;
    DFD_REQUIRE(layout->row_stride >= heads * HD && layout->frame_stride > 0 && layout->row_stride % per16 == 0 &&
                    layout->frame_stride % per16 == 0,
                "dfd_decoder_attn_map: key layout: row stride %lld, frame stride %lld (elements; rows must stay 16-byte aligned)",
                (long long)layout->row_stride, (long long)layout->frame_stride);
    DFD_REQUIRE(!layout->pos || dfd_aligned16(layout->pos), "dfd_decoder_attn_map: the positional embedding must be 16-byte aligned");
  }
  if (B == 0) return DFD_OK;
  const KvLayout lay = dfd_kv_layout(layout, patches, heads * HD);
  const FastDiv divp = FastDiv::make((uint32_t)patches);
  const int R = map_rows_per_block(heads);
  const int threads = heads * 8 * R;
  DFD_REQUIRE(threads <= 1024, "dfd_decoder_attn_map: heads=%d needs %d threads", heads, threads);
  const int S = T * patches;
  // keys per workgroup: up to 4 trips of 8R rows, fewer while the LDS (weights + staged positional rows) exceeds 64 KB
  // or the clip has no more rows
  int trips = 4;
  size_t lds = 0;
  int per = 0;
  for (;; --trips) {
    per = UN * R * trips;
    const int span = lay.pos ? (per + patches - 2) / patches + 1 : 0;  // frames a block's rows can touch
    lds = (size_t)2 * heads * per * sizeof(float) + (size_t)(span < T ? span : T) * heads * HD * sizeof(float);
    if (trips == 1 || (lds <= 64 * 1024 && UN * R * (trips - 1) < S)) break;
  }
  DFD_REQUIRE(lds <= 160 * 1024, "dfd_decoder_attn_map: %zu B of LDS", lds);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((S + per - 1) / per, B), block(threads);
  const int64_t branch_stride = (int64_t)B * heads * S;
#define MAP_LAUNCH1(KT, MT, PS)                                                                                       \
  do {                                                                                                                \
    if (lds > 64 * 1024)                                                                                              \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&decoder_attn_map_kernel<KT, MT, PS>),                  \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                \
    hipLaunchKernelGGL((decoder_attn_map_kernel<KT, MT, PS>), grid, block, lds, st, q, static_cast<const KT*>(k), frame_mask, \
                       stats, ext_weights, aff, branches, branch_stride, per, T, patches, heads, R, lay, divp);       \
  } while (0)
#define MAP_LAUNCH(KT, MT)                                                                \
  do {                                                                                    \
    if (lay.pos) MAP_LAUNCH1(KT, MT, true); else MAP_LAUNCH1(KT, MT, false);              \
  } while (0)
  if (kv_dtype == DFD_F32) { if (threads <= 512) MAP_LAUNCH(float, 512); else MAP_LAUNCH(float, 1024); }
  else { if (threads <= 512) MAP_LAUNCH(bf16_t, 512); else MAP_LAUNCH(bf16_t, 1024); }
#undef MAP_LAUNCH
#undef MAP_LAUNCH1
  DFD_CHECK_LAUNCH("dfd_decoder_attn_map");
  return DFD_OK;
}
