/* dfdclip_yuv.h — 8-bit YUV 4:2:0 sources for libdfdclip_hip.so: what video decoders actually deliver (NV12 from the hardware
 * decoder, I420 from ffmpeg; 1.5 bytes per pixel), taken where frames enter:
 *   dfd_yuv420_to_rgb_u8    pre-cropped clips -> the planar uint8 RGB that dfd_preprocess_u8, dfd_augment_u8,
 *                           dfd_elastic_remap_u8 and Detector.predict take;
 *   dfd_align_crop_yuv420   full frames -> face-aligned crops: dfd_align_crop_u8 (dfdclip_align.h) with the conversion fused
 *                           into its taps, so that only the pixels a crop touches are ever converted.
 * Added beside the C ABI of dfdclip.h WITHOUT a new DFD_ABI_VERSION (still 17): no other header changed.  A library built
 * before it lacks the symbols, which the loader reports by name.  Conventions (device pointers, `stream`, return codes,
 * dfd_last_error) are dfdclip.h's.  The Python binding lists the entry points in capi.YUV_SIGNATURES; tests/test_yuv_cpu.py
 * checks header, table and record sizes against each other, tests/test_hip_yuv.py the kernels against the integer
 * restatement in dfd-clip_amd/yuv.py, bit for bit.
 *
 * Arithmetic.  A sample (Y, U, V) becomes RGB with one matrix per call, in Q16; everything is 32-bit two's-complement
 * integer arithmetic with arithmetic shifts:
 *   y = Y - y_off;  u = U - 128;  v = V - 128
 *   R = clamp8((cy*y          + crv*v + 32768) >> 16)
 *   G = clamp8((cy*y + cgu*u  + cgv*v + 32768) >> 16)
 *   B = clamp8((cy*y + cbu*u          + 32768) >> 16)          clamp8(t) = min(max(t, 0), 255)
 * y is NOT clamped at 0: the final clamp does that work.  Chroma is replicated, not interpolated: the chroma sample of
 * pixel (r, c) of a buffer is sample (r >> 1, c >> 1) of its chroma planes; a buffer of H x W pixels has
 * ceil(H/2) x ceil(W/2) chroma samples, so odd sizes are legal.
 *
 * NOT pinned: the pixel values of swscale or cv2.cvtColor.  Neither is a dependency, so nothing here checks their bits;
 * OpenCV, for one, clamps Y - 16 at 0 and shifts by 20 bits where this shifts by 16. */
#ifndef DFDCLIP_YUV_H
#define DFDCLIP_YUV_H

#include <stdint.h>

#include "dfdclip.h"
#include "dfdclip_align.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The conversion matrix: plain HOST data, 32 bytes, read during the call.  The coefficients are Q16, e.g. BT.601 limited
 * range = {16, 76309, 104597, -25675, -53279, 132201}.  y_off must lie in 0..255 and every |coefficient| must be <= 2^21
 * (DFD_YUV_COEF_MAX), so that three products with samples of at most 255 plus the rounding term fit 32 bits. */
typedef struct dfd_yuv_matrix {
  int32_t y_off;
  int32_t cy, crv, cgu, cgv, cbu;
  int32_t reserved[2]; /* 0 */
} dfd_yuv_matrix_t;

#define DFD_YUV_MATRIX_BYTES 32
#define DFD_YUV_COEF_MAX 2097152

/* The source: plain HOST data, 64 bytes, read during the call; its pointers are device pointers.  One description serves
 * every 8-bit 4:2:0 layout, without a layout enum:
 *   NV12  u = uv, v = uv + 1, c_px_stride = 2          NV21  u = vu + 1, v = vu, c_px_stride = 2
 *   I420  u and v their own planes, c_px_stride = 1    YV12  likewise (only the order in memory differs)
 * Luma sample (r, c) of frame f is y[f * y_frame_stride + r * y_row_stride + c]; chroma sample (r, c) of frame f is
 * u[f * c_frame_stride + r * c_row_stride + c * c_px_stride], v likewise.  Strides are in bytes; padding is allowed; any
 * alignment of the pointers and strides is accepted.  y_row_stride >= win_w, c_row_stride >= the bytes one chroma row of
 * ONE plane spans ((ceil(win_w/2) - 1) * c_px_stride + 1), and a frame stride >= the bytes one frame's plane spans.  No row
 * padding is read, and nothing is read behind the last sample of the last row of a plane (for NV12 / NV21 the last byte of
 * the interleaved plane is the last sample of its second component). */
typedef struct dfd_yuv420 {
  const uint8_t* y;
  const uint8_t* u;
  const uint8_t* v;
  int64_t y_row_stride, y_frame_stride;
  int64_t c_row_stride, c_frame_stride;
  int32_t c_px_stride; /* 1 planar, 2 interleaved */
  int32_t reserved;    /* 0 */
} dfd_yuv420_t;

#define DFD_YUV420_BYTES 64

/* out[f] = frame f of `src` as RGB.
 *   src            n_frames buffers of win_h x win_w pixels (above)
 *   out            u8 planar [n_frames, 3, win_h, win_w] on the device, dense; must not overlap any of the three planes
 *   matrix         the conversion (above)
 * One streaming launch, no workspace, no atomics, no LDS: a lane owns eight pixels of two rows and their four chroma
 * samples, with 8-byte accesses where addresses allow and bytewise ones elsewhere; every byte of `out` is written exactly
 * once.  win_h * win_w < 2^31.  n_frames == 0 is a successful no-op. */
int dfd_yuv420_to_rgb_u8(const dfd_yuv420_t* src, int win_h, int win_w, uint8_t* out, int n_frames, const dfd_yuv_matrix_t* matrix,
                         void* stream);

/* out[f] = the out_h x out_w cut of frame f warped onto the canvas: dfd_align_crop_u8 of dfdclip_align.h on a 4:2:0
 * source.  A tap is CONVERTED FIRST AND BLENDED SECOND, so by definition the result is, bit for bit, that of
 * dfd_yuv420_to_rgb_u8 followed by dfd_align_crop_u8(layout = DFD_ALIGN_CHW, flags = 0) on the same records.  `frames` are
 * the 72-byte dfd_align_frame_t records (on the device, 8-byte aligned); `border`, DFD_ALIGN_FRAME_INVALID, the window check in
 * 64 bits and the Q16 / 1/32-pixel / 15-bit-weight arithmetic are dfdclip_align.h's, unchanged.  A tap outside the window is
 * `border` in all three channels and is not loaded, neither luma nor chroma, so no record can make the kernel read outside
 * the buffers.  The chroma of window pixel (r, c) is chroma sample (r >> 1, c >> 1) OF THE BUFFER: a window cut out of a
 * larger frame must start on even full-frame coordinates for that to be the frame's chroma (the kernel cannot check it; the
 * Python side does).  out is u8 planar [n_frames, 3, out_h, out_w], dense, and must not overlap any of the three planes.
 * One launch, no workspace, no atomics, no LDS; every byte of `out` is written exactly once.  n_frames == 0 is a successful
 * no-op. */
int dfd_align_crop_yuv420(const dfd_yuv420_t* src, int win_h, int win_w, uint8_t* out, int n_frames, int out_h, int out_w,
                          const dfd_align_frame_t* frames, const dfd_yuv_matrix_t* matrix, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_YUV_H */
