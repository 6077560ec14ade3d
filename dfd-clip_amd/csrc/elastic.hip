// Elastic warp of uint8 clips (include/dfdclip_elastic.h): the reference's self-supervised fakes (`ssl_fake`,
// src/datasets.py:401-418) in two launches.  The field kernel draws uniform noise with Philox, blurs it with a separable
// Q15 filter and scales it into a displacement field on a 1/32-pixel grid; the remap kernel samples every frame and channel
// of a clip bilinearly at the displaced positions.  Every step is integer, so dfd-clip_amd/elastic.py restates both bit
// for bit.
//
// Field kernel: a 256-thread workgroup owns a 32 x 64 tile of one field and both of its components.  The horizontal pass
// needs the tile's rows plus `radius` rows above and below; they are made 16 at a time: one Philox block per aligned
// group of eight noise elements goes into LDS by SOURCE column, a second pass lays the row out by tile column with the
// `reflect` boundary applied once per element (not once per tap), and the filter slides over that.  The vertical pass
// reads the tile's column of horizontal results from LDS.  The taps travel in the kernel arguments and are copied into LDS
// once: a lane filters four (vertical pass: eight) pixels at a time, so each broadcast tap read serves as many
// multiply-adds.  The two components end in registers and leave as one dword per pixel.
//
// Remap kernel: a lane owns four consecutive bytes of the flattened plane, as in align.hip.  Tap offsets and weights depend
// on the clip's field only, so the lane computes them once and loops over the frames of its chunk and the three channels:
// eight two-byte loads (a row's two taps are neighbouring bytes; served by L1 / L2) and one dword store per plane.
// Planes whose size is no multiple of 4 put some groups on odd addresses and leave a short last group: those are stored
// bytewise.  `reflect_101` brings every tap inside the frame whatever the field holds; that is what keeps the loads inside
// the buffer.  A clip without a field is copied by the same lanes.
#include "common.hpp"
#include "dropout.hpp"

#include "../../include/dfdclip_elastic.h"

namespace {

constexpr int kTileH = 32, kTileW = 64;  // field tile; 256 threads hold 8 pixels each
constexpr int kRowChunk = 16;            // rows of noise staged at a time
constexpr int kFrameChunk = 4;           // frames of a clip one remap workgroup walks

struct FieldArgs {
  uint32_t* field;  // (dx5, dy5) as one dword per pixel, dx5 in the low half
  const int64_t* field_ids;
  uint32_t key_lo, key_hi;
  int h, w, radius, tiles_x;
  int32_t alpha_q;
  int32_t taps[2 * DFD_ELASTIC_MAX_RADIUS + 1];
};

struct RemapArgs {
  const uint8_t* in;
  uint8_t* out;
  const uint32_t* field;
  const int32_t* field_of_clip;
  int n_frames, n_fields, w;
  int plane;             // h * w
  int groups;            // ceil(plane / 4)
  int blocks_per_plane;  // ceil(groups / 256)
  int chunks;            // ceil(n_frames / kFrameChunk)
};

// d c b a | a b c d | d c b a
__device__ __forceinline__ int reflect_edge(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// d c b | a b c d | c b a
__device__ __forceinline__ int reflect_101(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

__device__ __forceinline__ void store_u32(uint8_t* p, uint32_t v) { *reinterpret_cast<uint32_t*>(p) = v; }

__device__ __forceinline__ void store_group(uint8_t* p, uint32_t v, int nv) {
  if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    store_u32(p, v);
  } else {
    for (int k = 0; k < nv; ++k) p[k] = (uint8_t)(v >> (8 * k));
  }
}

__global__ __launch_bounds__(256) void elastic_field_kernel(FieldArgs a) {
  extern __shared__ int16_t lds[];
  const int R = a.radius, taps = 2 * R + 1;
  const int seg = kTileW + 2 * R;                 // columns a tile row's filter touches
  int16_t* hbuf = lds;                            // [kTileH + 2R][kTileW] horizontal results
  int16_t* src = hbuf + (kTileH + 2 * R) * kTileW;  // [kRowChunk][seg] noise at source columns lo ..
  int16_t* win = src + kRowChunk * seg;           // [kRowChunk][seg] noise at columns x0 - R .., boundary applied
  int32_t* tap = reinterpret_cast<int32_t*>(win + kRowChunk * seg);  // [taps]: a broadcast read per tap, shared by a lane's pixels
  const int tid = threadIdx.x, f = blockIdx.y;
  const int lx = tid % kTileW, lq = tid / kTileW;  // a lane's column, and its row modulo 4, in both filter passes
  for (int k = tid; k < taps; k += 256) tap[k] = a.taps[k];
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int x0 = tile_x * kTileW, y0 = tile_y * kTileH;
  const int ncols = min(kTileW, a.w - x0), nout = min(kTileH, a.h - y0);
  // every reflected column of [x0 - R, x0 + ncols + R) lies in [lo, hi], and hi - lo < seg
  const int lo = max(x0 - R, 0), hi = min(x0 + ncols - 1 + R, a.w - 1);
  const int span = hi - lo + 1;
  const int used = ncols + 2 * R, nrows = nout + 2 * R;
  const int gpr = (seg + 7) / 8 + 1;  // aligned groups of 8 that can touch a row's span
  const uint64_t id = (uint64_t)a.field_ids[f];
  const uint2 key{a.key_lo, a.key_hi};
  int v0[8], v1[8];
  for (int c = 0; c < 2; ++c) {
    for (int r0 = 0; r0 < nrows; r0 += kRowChunk) {
      const int nr = min(kRowChunk, nrows - r0);
      for (int i = tid; i < nr * gpr; i += 256) {
        const int r = i / gpr, j = i - r * gpr;
        const int yy = reflect_edge(y0 - R + r0 + r, a.h);
        const int64_t e_lo = ((int64_t)c * a.h + yy) * a.w + lo;
        const uint64_t g = (uint64_t)(e_lo >> 3) + j;
        const int pos0 = (int)((int64_t)(g << 3) - e_lo);  // -7 .. : where the group's first element falls in the span
        if (pos0 < span) {
          const uint4 d = dfd_philox4x32_10(uint4{(uint32_t)g, (uint32_t)(g >> 32), (uint32_t)id, (uint32_t)(id >> 32)}, key);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int pos = pos0 + k;
            if (pos >= 0 && pos < span) src[r * seg + pos] = (int16_t)((int)dfd_draw16(d, k) - 32768);
          }
        }
      }
      __syncthreads();
      for (int i = tid; i < nr * used; i += 256) {
        const int r = i / used, p = i - r * used;
        win[r * seg + p] = src[r * seg + reflect_edge(x0 - R + p, a.w) - lo];
      }
      __syncthreads();
      if (lx < ncols) {  // rows lq, lq + 4, lq + 8, lq + 12 of the chunk; a row beyond nr reads stale noise and is dropped
        const int16_t* row = win + lq * seg + lx;
        int acc[kRowChunk / 4];
#pragma unroll
        for (int m = 0; m < kRowChunk / 4; ++m) acc[m] = 1 << 14;
        for (int k = 0; k < taps; ++k) {
          const int q = tap[k];
#pragma unroll
          for (int m = 0; m < kRowChunk / 4; ++m) acc[m] += q * row[4 * m * seg + k];
        }
#pragma unroll
        for (int m = 0; m < kRowChunk / 4; ++m)
          if (lq + 4 * m < nr) hbuf[(r0 + lq + 4 * m) * kTileW + lx] = (int16_t)(acc[m] >> 15);
      }
      __syncthreads();
    }
    {  // rows lq, lq + 4, .. lq + 28 of the tile; rows beyond nout read stale results (still 16-bit: no overflow) and are dropped
      int acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0;
      if (lx < ncols) {
        const int16_t* col = hbuf + lq * kTileW + lx;
        for (int k = 0; k < taps; ++k) {
          const int q = tap[k];
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += q * col[(4 * j + k) * kTileW];
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t s = ((int64_t)acc[j] * a.alpha_q + (1ll << 32)) >> 33;
        const int d5 = (int)min(max(s, (int64_t)-32768), (int64_t)32767);
        if (c == 0) v0[j] = d5; else v1[j] = d5;
      }
    }
    __syncthreads();  // hbuf is rewritten for the second component
  }
  uint32_t* out = a.field + (int64_t)f * a.h * a.w;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = tid + 256 * j, ty = i / kTileW, x = i - ty * kTileW;
    if (ty < nout && x < ncols) out[(int64_t)(y0 + ty) * a.w + x0 + x] = ((uint32_t)v0[j] & 0xffffu) | ((uint32_t)v1[j] << 16);
  }
}

// the bytes at p and p + 1, at any alignment
__device__ __forceinline__ uint32_t load_pair(const uint8_t* p) {
  uint16_t v;
  __builtin_memcpy(&v, p, 2);
  return v;
}

// kPair (w >= 2): reflect_101 maps neighbouring indices to neighbouring columns, so a row's two taps are the two bytes at
// the smaller column and come in one 16-bit load; w == 1 has one column and loads it alone.
template <bool kPair>
__global__ __launch_bounds__(256) void elastic_remap_u8_kernel(RemapArgs a) {
  const int per_clip = a.chunks * a.blocks_per_plane;
  const int b = blockIdx.x / per_clip;
  const int rem = blockIdx.x - b * per_clip;
  const int chunk = rem / a.blocks_per_plane;
  const int g = (rem - chunk * a.blocks_per_plane) * 256 + threadIdx.x;
  if (g >= a.groups) return;
  const int e0 = 4 * g;
  const int nv = min(4, a.plane - e0);
  const int t0 = chunk * kFrameChunk;
  const int frames = min(t0 + kFrameChunk, a.n_frames) - t0;
  const int64_t base = ((int64_t)b * a.n_frames + t0) * 3 * a.plane;
  const uint8_t* src = a.in + base;
  uint8_t* dst = a.out + base + e0;
  const int fi = a.field_of_clip[b];
  if (fi < 0 || fi >= a.n_fields) {  // no field: the clip is copied
    for (int p = 0; p < 3 * frames; ++p) {
      const uint8_t* s = src + (int64_t)p * a.plane + e0;
      uint8_t* d = dst + (int64_t)p * a.plane;
      if (nv == 4 && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 3) == 0) {
        store_u32(d, *reinterpret_cast<const uint32_t*>(s));
      } else {
        for (int k = 0; k < nv; ++k) d[k] = s[k];
      }
    }
    return;
  }
  const uint32_t* fl = a.field + (int64_t)fi * a.plane + e0;
  const int h = a.plane / a.w;
  int y = e0 / a.w, x = e0 - y * a.w;
  // per pixel: the two rows' offsets of the smaller column, the weight of the byte there (the other byte's is 32 - wl) and
  // fy; a pixel beyond the plane's end keeps offset 0 and is not stored
  int oa[4], ob[4], wl[4], wy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    oa[k] = ob[k] = wl[k] = wy[k] = 0;
    if (k < nv) {
      const uint32_t d = fl[k];
      const int x5 = 32 * x + (int)(int16_t)(d & 0xffffu), y5 = 32 * y + (int)(int16_t)(d >> 16);
      const int fx = x5 & 31;
      const int xa = reflect_101(x5 >> 5, a.w), xb = reflect_101((x5 >> 5) + 1, a.w);
      const int ya = reflect_101(y5 >> 5, h) * a.w, yb = reflect_101((y5 >> 5) + 1, h) * a.w;
      const int xl = min(xa, xb);  // xb == xa +- 1 (w >= 2) or xa == xb == 0 (w == 1)
      oa[k] = ya + xl;
      ob[k] = yb + xl;
      wl[k] = xb < xa ? fx : 32 - fx;
      wy[k] = y5 & 31;
      if (++x == a.w) {
        x = 0;
        ++y;
      }
    }
  }
  for (int t = 0; t < frames; ++t) {
    uint32_t v[3] = {0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint8_t* s = src + (int64_t)(3 * t + c) * a.plane;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int ra, rb;  // the two rows, each 32 times its interpolated value
        if (kPair) {
          const uint32_t pa = load_pair(s + oa[k]), pb = load_pair(s + ob[k]);
          ra = wl[k] * (int)(pa & 0xffu) + (32 - wl[k]) * (int)(pa >> 8);
          rb = wl[k] * (int)(pb & 0xffu) + (32 - wl[k]) * (int)(pb >> 8);
        } else {
          ra = 32 * (int)s[oa[k]];
          rb = 32 * (int)s[ob[k]];
        }
        v[c] |= (uint32_t)((512 + (32 - wy[k]) * ra + wy[k] * rb) >> 10) << (8 * k);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) store_group(dst + (int64_t)(3 * t + c) * a.plane, v[c], nv);
  }
}

}  // namespace

extern "C" int dfd_elastic_field(int16_t* field, int n_fields, int h, int w, const int64_t* field_ids, uint64_t seed, const int32_t* taps,
                                 int radius, int32_t alpha_q, void* stream) {
  DFD_REQUIRE(n_fields >= 0, "dfd_elastic_field: bad field count %d", n_fields);
  DFD_REQUIRE(h > 0 && w > 0 && h <= DFD_ELASTIC_MAX_SIDE && w <= DFD_ELASTIC_MAX_SIDE && (int64_t)h * w < (1ll << 31),
              "dfd_elastic_field: bad size %dx%d", h, w);
  DFD_REQUIRE(radius >= 0 && radius <= DFD_ELASTIC_MAX_RADIUS, "dfd_elastic_field: bad radius %d (0..%d)", radius, DFD_ELASTIC_MAX_RADIUS);
  DFD_REQUIRE(taps, "dfd_elastic_field: null pointer (taps)");
  FieldArgs a;
  int64_t sum = 0;
  for (int k = 0; k < 2 * radius + 1; ++k) {
    DFD_REQUIRE(taps[k] >= 0, "dfd_elastic_field: tap %d is negative (%d)", k, taps[k]);
    sum += taps[k];
    a.taps[k] = taps[k];
  }
  for (int k = 2 * radius + 1; k < 2 * DFD_ELASTIC_MAX_RADIUS + 1; ++k) a.taps[k] = 0;
  DFD_REQUIRE(sum == DFD_ELASTIC_TAP_ONE, "dfd_elastic_field: the taps sum to %lld, not to %d", (long long)sum, DFD_ELASTIC_TAP_ONE);
  if (n_fields == 0) return DFD_OK;
  DFD_REQUIRE(field && field_ids, "dfd_elastic_field: null pointer");
  DFD_REQUIRE((reinterpret_cast<uintptr_t>(field) & 3) == 0, "dfd_elastic_field: the field must be 4-byte aligned");
  DFD_REQUIRE((reinterpret_cast<uintptr_t>(field_ids) & 7) == 0, "dfd_elastic_field: the field ids must be 8-byte aligned");
  DFD_REQUIRE(n_fields <= 65535, "dfd_elastic_field: too many fields (%d)", n_fields);
  a.field = reinterpret_cast<uint32_t*>(field);
  a.field_ids = field_ids;
  a.key_lo = (uint32_t)seed ^ DFD_ELASTIC_SITE;
  a.key_hi = (uint32_t)(seed >> 32);
  a.h = h;
  a.w = w;
  a.radius = radius;
  a.tiles_x = (w + kTileW - 1) / kTileW;
  a.alpha_q = alpha_q;
  const int64_t tiles = (int64_t)a.tiles_x * ((h + kTileH - 1) / kTileH);
  DFD_REQUIRE(tiles < (1ll << 31), "dfd_elastic_field: too many tiles (%lld)", (long long)tiles);
  const int seg = kTileW + 2 * radius;
  const size_t lds = sizeof(int16_t) * ((size_t)(kTileH + 2 * radius) * kTileW + 2 * (size_t)kRowChunk * seg) +
                     sizeof(int32_t) * (2 * (size_t)radius + 1);  // 17,604 B at radius 24; 58,372 B at radius 128
  hipLaunchKernelGGL(elastic_field_kernel, dim3((unsigned)tiles, (unsigned)n_fields), dim3(256), lds, static_cast<hipStream_t>(stream), a);
  DFD_CHECK_LAUNCH("dfd_elastic_field");
  return DFD_OK;
}

extern "C" int dfd_elastic_remap_u8(const uint8_t* in, uint8_t* out, int n_clips, int n_frames, int h, int w, const int16_t* field,
                                    int n_fields, const int32_t* field_of_clip, void* stream) {
  DFD_REQUIRE(n_clips >= 0 && n_frames >= 0, "dfd_elastic_remap_u8: bad clip or frame count %d x %d", n_clips, n_frames);
  DFD_REQUIRE(n_fields >= 0, "dfd_elastic_remap_u8: bad field count %d", n_fields);
  DFD_REQUIRE(h > 0 && w > 0 && h <= DFD_ELASTIC_MAX_SIDE && w <= DFD_ELASTIC_MAX_SIDE && (int64_t)h * w < (1ll << 31),
              "dfd_elastic_remap_u8: bad size %dx%d", h, w);
  if (n_clips == 0 || n_frames == 0) return DFD_OK;
  DFD_REQUIRE(in && out && field_of_clip, "dfd_elastic_remap_u8: null pointer");
  DFD_REQUIRE(field || n_fields == 0, "dfd_elastic_remap_u8: %d fields but a null field pointer", n_fields);
  DFD_REQUIRE((reinterpret_cast<uintptr_t>(field) & 3) == 0, "dfd_elastic_remap_u8: the field must be 4-byte aligned");
  RemapArgs a;
  a.plane = h * w;
  const int64_t frames = (int64_t)n_clips * n_frames;
  DFD_REQUIRE(frames <= (1ll << 60) / (3 * (int64_t)a.plane), "dfd_elastic_remap_u8: %lld frames of %dx%d are out of range", (long long)frames, h, w);
  const int64_t bytes = frames * 3 * a.plane;
  DFD_REQUIRE(in + bytes <= out || out + bytes <= in, "dfd_elastic_remap_u8: in and out overlap; the warp is not made in place");
  a.in = in;
  a.out = out;
  a.field = reinterpret_cast<const uint32_t*>(field);
  a.field_of_clip = field_of_clip;
  a.n_frames = n_frames;
  a.n_fields = n_fields;
  a.w = w;
  a.groups = (int)(((int64_t)a.plane + 3) / 4);
  a.blocks_per_plane = (a.groups + 255) / 256;
  a.chunks = (n_frames + kFrameChunk - 1) / kFrameChunk;
  const int64_t blocks = (int64_t)n_clips * a.chunks * a.blocks_per_plane;
  DFD_REQUIRE(blocks < (1ll << 31), "dfd_elastic_remap_u8: too many blocks (%lld)", (long long)blocks);
  if (w >= 2) {
    hipLaunchKernelGGL(elastic_remap_u8_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  } else {
    hipLaunchKernelGGL(elastic_remap_u8_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  }
  DFD_CHECK_LAUNCH("dfd_elastic_remap_u8");
  return DFD_OK;
}
