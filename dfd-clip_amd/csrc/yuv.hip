// 8-bit YUV 4:2:0 sources (include/dfdclip_yuv.h): NV12 / NV21 / I420 / YV12 through one description of three planes.
//   yuv420_to_rgb_u8_kernel      whole buffers -> planar RGB, streaming
//   yuv420_align_crop_kernel     align.hip's gather with the conversion in its taps (converted first, blended second)
// Every step is 32-bit integer (the affine part of the gather 64-bit, as in align.hip), so dfd-clip_amd/yuv.py restates both
// bit for bit.  No LDS, no atomics, no workspace.
//
// Converter, work split: a lane owns eight consecutive pixels of rows 2r and 2r+1 and the four chroma samples they share:
// two 8-byte luma loads, one 8-byte load of an interleaved chroma plane or two 4-byte loads of planar ones, six 8-byte
// stores.  An access takes the wide form when its address is aligned to its size and the lane's run is whole; otherwise
// (odd bases, odd strides, the last columns of a row) it goes bytewise over exactly the bytes that exist, so no padding and
// nothing behind a plane's last sample is read.  The chroma terms of the matrix are computed once per chroma sample.
//
// Gather: the straightforward form, not tuned: each of the four taps loads its own Y, U and V bytes (two horizontal taps
// share a chroma sample when sx is even; the loads hit the same L1 line either way) and converts them.  A tap is loaded only
// after its position was checked against the window in 64 bits.
#include "common.hpp"

#include "../../include/dfdclip_yuv.h"

namespace {

struct YuvSrc {
  const uint8_t *y, *u, *v;
  int64_t y_rs, y_fs, c_rs, c_fs;  // bytes
  int c_px;                        // 1 planar, 2 interleaved
  int pair;                        // interleaved with adjacent pointers: 1 = v == u + 1 (NV12), 2 = u == v + 1 (NV21), else 0
};

struct YuvMat {
  int y_off, cy, crv, cgu, cgv, cbu;
};

struct ConvArgs {
  YuvSrc s;
  YuvMat m;
  uint8_t* out;
  int h, w;
  int gw;                // ceil(w / 8): lanes per row pair
  int groups;            // ceil(h / 2) * gw
  int blocks_per_frame;  // ceil(groups / 256)
};

struct CropArgs {
  YuvSrc s;
  YuvMat m;
  uint8_t* out;
  const dfd_align_frame_t* frames;
  int win_h, win_w, out_w;
  int plane;             // out_h * out_w
  int groups;            // ceil(plane / 4)
  int blocks_per_frame;  // ceil(groups / 256)
};

__device__ __forceinline__ int clamp8(int t) { return min(max(t, 0), 255); }

// A clamped sample on its way into a packed word.  hipcc (ROCm 7.2) fuses `clamp8(a >> 16) | clamp8(b >> 16) << 8` into one
// v_ashr_pk_u8_i32 and ORs the word's other bytes into the upper half of its result as if that half were zero; on gfx950 the
// instruction leaves the destination's upper 16 bits as they were, and here the destination was the register of `b`: bytes
// 2 and 3 of every packed dword came out OR-ed with bits of the unshifted sum (seen on the device, read in the assembly).
// An empty asm hides where the value came from, so the fusion cannot form; it emits nothing.  tools/isa_lint.py refuses
// the instruction in any kernel.
__device__ __forceinline__ uint64_t packable(int v) {
  asm("" : "+v"(v));
  return (uint64_t)(uint32_t)v;
}

// n <= 8 bytes from p, byte k in bits 8k..8k+7
__device__ __forceinline__ uint64_t load_run8(const uint8_t* p, int n) {
  if (n == 8 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) return *reinterpret_cast<const uint64_t*>(p);
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < n) v |= (uint64_t)p[k] << (8 * k);
  return v;
}

// n <= 4 samples `stride` bytes apart
__device__ __forceinline__ uint32_t load_run4(const uint8_t* p, int n, int stride) {
  if (n == 4 && stride == 1 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n) v |= (uint32_t)p[k * stride] << (8 * k);
  return v;
}

__device__ __forceinline__ void store_run8(uint8_t* p, uint64_t v, int n) {
  if (n == 8 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
    *reinterpret_cast<uint64_t*>(p) = v;
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (k < n) p[k] = (uint8_t)(v >> (8 * k));
}

// bytes 0, 2, 4, 6 of w in bytes 0..3
__device__ __forceinline__ uint32_t even_bytes(uint64_t w) {
  return (uint32_t)(w & 255) | (uint32_t)((w >> 8) & 0xff00) | (uint32_t)((w >> 16) & 0xff0000) | (uint32_t)((w >> 24) & 0xff000000u);
}

__global__ __launch_bounds__(256) void yuv420_to_rgb_u8_kernel(ConvArgs a) {
  const int f = blockIdx.x / a.blocks_per_frame;
  const int g = (blockIdx.x - f * a.blocks_per_frame) * 256 + threadIdx.x;
  if (g >= a.groups) return;
  const int rp = g / a.gw, cg = g - rp * a.gw;
  const int r0 = 2 * rp, c0 = 8 * cg;
  const int nv = min(8, a.w - c0);  // pixels of this lane's run, >= 1
  const int nc = (nv + 1) >> 1;     // and their chroma samples
  const bool two = r0 + 1 < a.h;

  const int64_t co = (int64_t)f * a.s.c_fs + (int64_t)rp * a.s.c_rs + (int64_t)(4 * cg) * a.s.c_px;
  uint32_t U, V;
  if (a.s.pair) {
    const uint64_t w = load_run8((a.s.pair == 1 ? a.s.u : a.s.v) + co, 2 * nc);
    const uint32_t first = even_bytes(w), second = even_bytes(w >> 8);
    U = a.s.pair == 1 ? first : second;
    V = a.s.pair == 1 ? second : first;
  } else {
    U = load_run4(a.s.u + co, nc, a.s.c_px);
    V = load_run4(a.s.v + co, nc, a.s.c_px);
  }
  const uint8_t* yp = a.s.y + (int64_t)f * a.s.y_fs + (int64_t)r0 * a.s.y_rs + c0;
  uint64_t Y[2];
  Y[0] = load_run8(yp, nv);
  Y[1] = two ? load_run8(yp + a.s.y_rs, nv) : 0ull;

  uint64_t px[2][3] = {{0ull, 0ull, 0ull}, {0ull, 0ull, 0ull}};
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // chroma sample j serves pixels 2j, 2j+1 of both rows (lanes past nv compute on zeros)
    const int u = (int)((U >> (8 * j)) & 255u) - 128, v = (int)((V >> (8 * j)) & 255u) - 128;
    const int tr = a.m.crv * v + 32768, tg = a.m.cgu * u + a.m.cgv * v + 32768, tb = a.m.cbu * u + 32768;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int k = 2 * j + d;
        const int t = a.m.cy * ((int)((Y[row] >> (8 * k)) & 255ull) - a.m.y_off);
        px[row][0] |= packable(clamp8((t + tr) >> 16)) << (8 * k);
        px[row][1] |= packable(clamp8((t + tg) >> 16)) << (8 * k);
        px[row][2] |= packable(clamp8((t + tb) >> 16)) << (8 * k);
      }
    }
  }
  const int64_t plane = (int64_t)a.h * a.w;
  uint8_t* o = a.out + (int64_t)f * 3 * plane + (int64_t)r0 * a.w + c0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    store_run8(o + c * plane, px[0][c], nv);
    if (two) store_run8(o + c * plane + a.w, px[1][c], nv);
  }
}

__device__ __forceinline__ void store_u32(uint8_t* p, uint32_t v) { *reinterpret_cast<uint32_t*>(p) = v; }

// align_crop_u8_kernel of align.hip (a lane owns four consecutive bytes of the flattened output plane in all three
// channels) with a 4:2:0 tap.
__global__ __launch_bounds__(256) void yuv420_align_crop_kernel(CropArgs a) {
  const int f = blockIdx.x / a.blocks_per_frame;
  const int g = (blockIdx.x - f * a.blocks_per_frame) * 256 + threadIdx.x;
  if (g >= a.groups) return;
  const dfd_align_frame_t* r = a.frames + f;
  const int e0 = 4 * g;
  const int nv = min(4, a.plane - e0);
  const int border = min(max(r->border, 0), 255);
  uint32_t px[3];
  if (r->flags & DFD_ALIGN_FRAME_INVALID) {
    px[0] = px[1] = px[2] = (uint32_t)border * 0x01010101u;
  } else {
    px[0] = px[1] = px[2] = 0u;
    const uint8_t* ys = a.s.y + (int64_t)f * a.s.y_fs;
    const uint8_t* us = a.s.u + (int64_t)f * a.s.c_fs;
    const uint8_t* vs = a.s.v + (int64_t)f * a.s.c_fs;
    // the affine part in unsigned 64-bit arithmetic, as in align.hip
    const uint64_t q0 = (uint64_t)r->q[0], q1 = (uint64_t)r->q[1], q3 = (uint64_t)r->q[3], q4 = (uint64_t)r->q[4];
    int i = e0 / a.out_w, j = e0 - i * a.out_w;
    const uint64_t X = (uint64_t)((int64_t)r->x0 + j), Y = (uint64_t)((int64_t)r->y0 + i);
    uint64_t xf = q0 * X + q1 * Y + (uint64_t)r->q[2];
    uint64_t yf = q3 * X + q4 * Y + (uint64_t)r->q[5];
    const uint64_t wrap_x = q1 - q0 * (uint64_t)(a.out_w - 1), wrap_y = q4 - q3 * (uint64_t)(a.out_w - 1);
    const int64_t win_x = r->win_x, win_y = r->win_y;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < nv) {
        const int64_t x5 = ((int64_t)(xf + 1024u)) >> 11, y5 = ((int64_t)(yf + 1024u)) >> 11;
        const int fx = (int)(x5 & 31), fy = (int)(y5 & 31);
        const int64_t rx = (x5 >> 5) - win_x, ry = (y5 >> 5) - win_y;  // tap (0, 0) relative to the window
        int acc[3] = {512, 512, 512};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int dx = t & 1, dy = t >> 1;
          const int w = (dx ? fx : 32 - fx) * (dy ? fy : 32 - fy);
          const int64_t tx = rx + dx, ty = ry + dy;
          if (tx >= 0 && tx < a.win_w && ty >= 0 && ty < a.win_h) {
            const int64_t co = (ty >> 1) * a.s.c_rs + (tx >> 1) * a.s.c_px;
            const int y = (int)ys[ty * a.s.y_rs + tx] - a.m.y_off;
            const int u = (int)us[co] - 128, v = (int)vs[co] - 128;
            const int l = a.m.cy * y;
            acc[0] += w * clamp8((l + a.m.crv * v + 32768) >> 16);
            acc[1] += w * clamp8((l + a.m.cgu * u + a.m.cgv * v + 32768) >> 16);
            acc[2] += w * clamp8((l + a.m.cbu * u + 32768) >> 16);
          } else {
            acc[0] += w * border;
            acc[1] += w * border;
            acc[2] += w * border;
          }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] |= (uint32_t)(acc[c] >> 10) << (8 * k);
        if (++j == a.out_w) {
          j = 0;
          xf += wrap_x;
          yf += wrap_y;
        } else {
          xf += q0;
          yf += q3;
        }
      }
    }
  }
  uint8_t* o = a.out + (int64_t)f * 3 * a.plane + e0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint8_t* oc = o + (int64_t)c * a.plane;
    if (nv == 4 && (reinterpret_cast<uintptr_t>(oc) & 3) == 0) {
      store_u32(oc, px[c]);
    } else {
      for (int k = 0; k < nv; ++k) oc[k] = (uint8_t)(px[c] >> (8 * k));
    }
  }
}

// The checks both entry points share, in dfd_align_crop_u8's order: counts and sizes, the host records, strides against row
// lengths; then (n_frames > 0 only) frame strides against frame spans, device pointers, overlap of `out` with each plane.
// `done` is set when n_frames == 0 passed the first half: nothing is left to do.
int check_source(const char* fn, const dfd_yuv420_t* src, int win_h, int win_w, const uint8_t* out, int64_t out_bytes, int n_frames,
                 const dfd_yuv_matrix_t* matrix, YuvSrc* s, YuvMat* m, bool* done) {
  *done = false;
  DFD_REQUIRE(n_frames >= 0, "%s: bad frame count %d", fn, n_frames);
  DFD_REQUIRE(win_h > 0 && win_w > 0, "%s: bad window size %dx%d", fn, win_h, win_w);
  DFD_REQUIRE(src && matrix, "%s: null source description or matrix", fn);
  DFD_REQUIRE(src->c_px_stride == 1 || src->c_px_stride == 2, "%s: chroma pixel stride %d is neither 1 (planar) nor 2 (interleaved)", fn,
              src->c_px_stride);
  DFD_REQUIRE(matrix->y_off >= 0 && matrix->y_off <= 255, "%s: matrix y_off %d lies outside 0..255", fn, matrix->y_off);
  const int32_t coef[5] = {matrix->cy, matrix->crv, matrix->cgu, matrix->cgv, matrix->cbu};
  for (int k = 0; k < 5; ++k)
    DFD_REQUIRE((int64_t)coef[k] >= -(int64_t)DFD_YUV_COEF_MAX && (int64_t)coef[k] <= (int64_t)DFD_YUV_COEF_MAX,
                "%s: matrix coefficient %d is out of range (|c| <= 2^21)", fn, coef[k]);
  const int ch = (win_h + 1) / 2, cw = (win_w + 1) / 2;
  const int64_t c_row_bytes = (int64_t)(cw - 1) * src->c_px_stride + 1;
  DFD_REQUIRE(src->y_row_stride >= win_w, "%s: luma row stride %lld is smaller than a row (%d bytes)", fn, (long long)src->y_row_stride, win_w);
  DFD_REQUIRE(src->c_row_stride >= c_row_bytes, "%s: chroma row stride %lld is smaller than a row (%lld bytes)", fn,
              (long long)src->c_row_stride, (long long)c_row_bytes);
  DFD_REQUIRE(src->y_row_stride <= (1ll << 60) / win_h && src->c_row_stride <= (1ll << 60) / win_h, "%s: row stride %lld / %lld is out of range",
              fn, (long long)src->y_row_stride, (long long)src->c_row_stride);
  if (n_frames == 0) {
    *done = true;
    return DFD_OK;
  }
  const int64_t y_span = (int64_t)(win_h - 1) * src->y_row_stride + win_w;  // first to last byte read of one frame's plane
  const int64_t c_span = (int64_t)(ch - 1) * src->c_row_stride + c_row_bytes;
  DFD_REQUIRE(src->y_frame_stride >= y_span && src->y_frame_stride <= (1ll << 62) / n_frames,
              "%s: luma frame stride %lld is smaller than a frame (%lld bytes) or out of range", fn, (long long)src->y_frame_stride, (long long)y_span);
  DFD_REQUIRE(src->c_frame_stride >= c_span && src->c_frame_stride <= (1ll << 62) / n_frames,
              "%s: chroma frame stride %lld is smaller than a frame (%lld bytes) or out of range", fn, (long long)src->c_frame_stride,
              (long long)c_span);
  DFD_REQUIRE(src->y && src->u && src->v && out, "%s: null pointer", fn);
  const int64_t y_bytes = (int64_t)(n_frames - 1) * src->y_frame_stride + y_span;
  const int64_t c_bytes = (int64_t)(n_frames - 1) * src->c_frame_stride + c_span;
  const uint8_t* planes[3] = {src->y, src->u, src->v};
  const int64_t bytes[3] = {y_bytes, c_bytes, c_bytes};
  const char* names[3] = {"y", "u", "v"};
  for (int k = 0; k < 3; ++k)
    DFD_REQUIRE(planes[k] + bytes[k] <= out || out + out_bytes <= planes[k], "%s: the %s plane and out overlap; the conversion is not made in place",
                fn, names[k]);
  s->y = src->y;
  s->u = src->u;
  s->v = src->v;
  s->y_rs = src->y_row_stride;
  s->y_fs = src->y_frame_stride;
  s->c_rs = src->c_row_stride;
  s->c_fs = src->c_frame_stride;
  s->c_px = src->c_px_stride;
  s->pair = src->c_px_stride == 2 ? (src->v == src->u + 1 ? 1 : src->u == src->v + 1 ? 2 : 0) : 0;
  m->y_off = matrix->y_off;
  m->cy = matrix->cy;
  m->crv = matrix->crv;
  m->cgu = matrix->cgu;
  m->cgv = matrix->cgv;
  m->cbu = matrix->cbu;
  return DFD_OK;
}

}  // namespace

extern "C" int dfd_yuv420_to_rgb_u8(const dfd_yuv420_t* src, int win_h, int win_w, uint8_t* out, int n_frames, const dfd_yuv_matrix_t* matrix,
                                    void* stream) {
  static_assert(sizeof(dfd_yuv_matrix_t) == DFD_YUV_MATRIX_BYTES, "dfd_yuv_matrix_t must stay 32 bytes");
  static_assert(sizeof(dfd_yuv420_t) == DFD_YUV420_BYTES, "dfd_yuv420_t must stay 64 bytes");
  DFD_REQUIRE(win_h <= 0 || win_w <= 0 || (int64_t)win_h * win_w < (1ll << 31), "dfd_yuv420_to_rgb_u8: bad window size %dx%d", win_h, win_w);
  ConvArgs a;
  bool done;
  const int64_t out_bytes = (int64_t)(n_frames > 0 ? n_frames : 0) * 3 * (win_h > 0 ? win_h : 0) * (win_w > 0 ? win_w : 0);
  const int rc = check_source("dfd_yuv420_to_rgb_u8", src, win_h, win_w, out, out_bytes, n_frames, matrix, &a.s, &a.m, &done);
  if (rc != DFD_OK || done) return rc;
  a.out = out;
  a.h = win_h;
  a.w = win_w;
  a.gw = (win_w + 7) / 8;
  a.groups = ((win_h + 1) / 2) * a.gw;
  a.blocks_per_frame = (a.groups + 255) / 256;
  const int64_t blocks = (int64_t)n_frames * a.blocks_per_frame;
  DFD_REQUIRE(blocks < (1ll << 31), "dfd_yuv420_to_rgb_u8: too many blocks (%lld)", (long long)blocks);
  hipLaunchKernelGGL(yuv420_to_rgb_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  DFD_CHECK_LAUNCH("dfd_yuv420_to_rgb_u8");
  return DFD_OK;
}

extern "C" int dfd_align_crop_yuv420(const dfd_yuv420_t* src, int win_h, int win_w, uint8_t* out, int n_frames, int out_h, int out_w,
                                     const dfd_align_frame_t* frames, const dfd_yuv_matrix_t* matrix, void* stream) {
  DFD_REQUIRE(out_h > 0 && out_w > 0 && (int64_t)out_h * out_w < (1ll << 31), "dfd_align_crop_yuv420: bad output size %dx%d", out_h, out_w);
  CropArgs a;
  bool done;
  const int64_t out_bytes = (int64_t)(n_frames > 0 ? n_frames : 0) * 3 * out_h * out_w;
  const int rc = check_source("dfd_align_crop_yuv420", src, win_h, win_w, out, out_bytes, n_frames, matrix, &a.s, &a.m, &done);
  if (rc != DFD_OK || done) return rc;
  DFD_REQUIRE(frames, "dfd_align_crop_yuv420: %d frames but no parameter records", n_frames);
  DFD_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 7) == 0, "dfd_align_crop_yuv420: the records must be 8-byte aligned");
  a.out = out;
  a.frames = frames;
  a.win_h = win_h;
  a.win_w = win_w;
  a.out_w = out_w;
  a.plane = out_h * out_w;
  a.groups = (a.plane + 3) / 4;
  a.blocks_per_frame = (a.groups + 255) / 256;
  const int64_t blocks = (int64_t)n_frames * a.blocks_per_frame;
  DFD_REQUIRE(blocks < (1ll << 31), "dfd_align_crop_yuv420: too many blocks (%lld)", (long long)blocks);
  hipLaunchKernelGGL(yuv420_align_crop_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  DFD_CHECK_LAUNCH("dfd_align_crop_yuv420");
  return DFD_OK;
}
