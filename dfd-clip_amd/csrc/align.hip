// Face-aligned crops from full frames (include/dfdclip_align.h): the reference's warp onto a 256x256 canvas followed by
// its 150x150 cut (pipeline.py:114-182), as one gather.  Only the cut is computed: output pixel (i, j) is canvas pixel
// (x0 + j, y0 + i), mapped back into the frame by the record's Q16 inverse matrix and sampled bilinearly on a 1/32-pixel
// grid.  Every step is integer, so dfd-clip_amd/align.py restates it bit for bit.
//
// Work split: a lane owns four consecutive bytes of a frame's flattened output plane, in all three channels, and stores
// them as one dword per channel (a 150x150 plane is 22,500 bytes, a multiple of 4; a group may straddle two rows).  Planes
// whose size is no multiple of 4 put some groups on odd addresses and leave a short last group: those are stored bytewise.
// The taps are byte loads served by L1/L2 (neighbouring lanes read neighbouring source pixels); there is no LDS stage.
// A tap is loaded only after its position was checked against the window, in 64 bits: that check is what keeps any
// record, however wild, inside the buffer.
#include "common.hpp"

#include "../../include/dfdclip_align.h"

namespace {

struct AlignArgs {
  const uint8_t* in;
  uint8_t* out;
  const dfd_align_frame_t* frames;
  int64_t row_stride, frame_stride, ch_stride;  // bytes; ch_stride: 1 interleaved, win_h * row_stride planar
  int px_stride;                                // 3 interleaved, 1 planar
  int win_h, win_w, out_w;
  int plane;             // out_h * out_w
  int groups;            // ceil(plane / 4)
  int blocks_per_frame;  // ceil(groups / 256)
  int swap_rb;
};

__device__ __forceinline__ void store_u32(uint8_t* p, uint32_t v) { *reinterpret_cast<uint32_t*>(p) = v; }

__global__ __launch_bounds__(256) void align_crop_u8_kernel(AlignArgs a) {
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
    const uint8_t* src = a.in + (int64_t)f * a.frame_stride;
    // the affine part in unsigned 64-bit arithmetic: exact while nothing overflows, wrapping (and still in step with the
    // restatement) where a record is absurd; stepping by q0 / q3 along a row is the same value in that ring
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
            const uint8_t* p = src + ty * a.row_stride + tx * a.px_stride;
            acc[0] += w * p[0];
            acc[1] += w * p[a.ch_stride];
            acc[2] += w * p[2 * a.ch_stride];
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
    uint8_t* oc = o + (int64_t)(a.swap_rb ? 2 - c : c) * a.plane;
    if (nv == 4 && (reinterpret_cast<uintptr_t>(oc) & 3) == 0) {
      store_u32(oc, px[c]);
    } else {
      for (int k = 0; k < nv; ++k) oc[k] = (uint8_t)(px[c] >> (8 * k));
    }
  }
}

}  // namespace

extern "C" int dfd_align_crop_u8(const uint8_t* in, int layout, int64_t row_stride, int64_t frame_stride, int win_h, int win_w,
                                 uint8_t* out, int n_frames, int out_h, int out_w, const dfd_align_frame_t* frames, uint32_t flags,
                                 void* stream) {
  static_assert(sizeof(dfd_align_frame_t) == DFD_ALIGN_FRAME_BYTES, "dfd_align_frame_t must stay 72 bytes");
  DFD_REQUIRE(layout == DFD_ALIGN_HWC || layout == DFD_ALIGN_CHW, "dfd_align_crop_u8: unknown layout %d", layout);
  DFD_REQUIRE((flags & ~DFD_ALIGN_SWAP_RB) == 0, "dfd_align_crop_u8: unknown flag bits 0x%x", flags & ~DFD_ALIGN_SWAP_RB);
  DFD_REQUIRE(n_frames >= 0, "dfd_align_crop_u8: bad frame count %d", n_frames);
  DFD_REQUIRE(win_h > 0 && win_w > 0, "dfd_align_crop_u8: bad window size %dx%d", win_h, win_w);
  DFD_REQUIRE(out_h > 0 && out_w > 0 && (int64_t)out_h * out_w < (1ll << 31), "dfd_align_crop_u8: bad output size %dx%d", out_h, out_w);
  const bool hwc = layout == DFD_ALIGN_HWC;
  const int64_t row_bytes = (int64_t)win_w * (hwc ? 3 : 1);
  DFD_REQUIRE(row_stride >= row_bytes, "dfd_align_crop_u8: row stride %lld is smaller than a row (%lld bytes)",
              (long long)row_stride, (long long)row_bytes);
  DFD_REQUIRE(row_stride <= (1ll << 60) / (3 * (int64_t)win_h), "dfd_align_crop_u8: row stride %lld is out of range", (long long)row_stride);
  if (n_frames == 0) return DFD_OK;
  const int64_t frame_bytes = ((int64_t)win_h * (hwc ? 1 : 3) - 1) * row_stride + row_bytes;  // first to last byte read
  DFD_REQUIRE(frame_stride >= frame_bytes && frame_stride <= (1ll << 62) / n_frames,
              "dfd_align_crop_u8: frame stride %lld is smaller than a frame (%lld bytes) or out of range", (long long)frame_stride,
              (long long)frame_bytes);
  DFD_REQUIRE(frames, "dfd_align_crop_u8: %d frames but no parameter records", n_frames);
  DFD_REQUIRE(in && out, "dfd_align_crop_u8: null pointer");
  DFD_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 7) == 0, "dfd_align_crop_u8: the records must be 8-byte aligned");
  const int64_t in_bytes = (int64_t)(n_frames - 1) * frame_stride + frame_bytes;
  const int64_t out_bytes = (int64_t)n_frames * 3 * out_h * out_w;
  DFD_REQUIRE(in + in_bytes <= out || out + out_bytes <= in, "dfd_align_crop_u8: in and out overlap; the crop is not made in place");
  AlignArgs a;
  a.in = in;
  a.out = out;
  a.frames = frames;
  a.row_stride = row_stride;
  a.frame_stride = frame_stride;
  a.ch_stride = hwc ? 1 : (int64_t)win_h * row_stride;
  a.px_stride = hwc ? 3 : 1;
  a.win_h = win_h;
  a.win_w = win_w;
  a.out_w = out_w;
  a.plane = out_h * out_w;
  a.groups = (a.plane + 3) / 4;
  a.blocks_per_frame = (a.groups + 255) / 256;
  a.swap_rb = (flags & DFD_ALIGN_SWAP_RB) ? 1 : 0;
  const int64_t blocks = (int64_t)n_frames * a.blocks_per_frame;
  DFD_REQUIRE(blocks < (1ll << 31), "dfd_align_crop_u8: too many blocks (%lld)", (long long)blocks);
  hipLaunchKernelGGL(align_crop_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  DFD_CHECK_LAUNCH("dfd_align_crop_u8");
  return DFD_OK;
}
