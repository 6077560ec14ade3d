/* dfdclip_align.h — device-side face alignment of libdfdclip_hip.so: the warp-and-cut stage the reference runs on the host
 * in front of every video (pipeline.py:114-182: `affine_transform`, `cut_patch`, `crop_patch`; the same code in
 * preprocessing/extract_faces.py:55-125), from full uint8 frames plus one parameter record per frame to the planar crops
 * that dfd_preprocess_u8, dfd_augment_u8 and Detector.predict take.  Added beside the C ABI of dfdclip.h WITHOUT a new
 * DFD_ABI_VERSION (still 17): nothing in dfdclip.h, dfdclip_ext.h, dfdclip_explain.h or dfdclip_augment.h changed.  A library
 * built before it lacks the symbol, which the loader reports by name.  Conventions (device pointers, `stream`, return
 * codes, dfd_last_error) are dfdclip.h's.
 *
 * It lives in a header of its own because the function lists of the other headers are pinned by their tests.  The Python
 * binding lists it in capi.ALIGN_SIGNATURES; tests/test_align_cpu.py checks header, table and record size against each
 * other, tests/test_hip_align.py the kernel against the integer restatement in dfd-clip_amd/align.py, bit for bit.
 *
 * NOT pinned: the pixel values of cv2.warpAffine.  The arithmetic below keeps its structure (INTER_LINEAR on a 1/32-pixel
 * grid with 15-bit weights, BORDER_CONSTANT), but OpenCV rounds each term of the coordinate at 1/1024 pixel where this
 * rounds their sum, and OpenCV is not a dependency, so nothing here checks its bits. */
#ifndef DFDCLIP_ALIGN_H
#define DFDCLIP_ALIGN_H

#include <stdint.h>

#include "dfdclip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `layout` of the source frames */
#define DFD_ALIGN_HWC 0 /* interleaved [win_h, win_w, 3]: what video decoders deliver */
#define DFD_ALIGN_CHW 1 /* planar [3, win_h, win_w]: plane c starts c * win_h * row_stride bytes into the frame */

/* `flags` of the call */
#define DFD_ALIGN_SWAP_RB 1u /* channels 0 and 2 are exchanged on the store (BGR -> RGB) */

/* `flags` of a record */
#define DFD_ALIGN_FRAME_INVALID 1u /* no face: the whole crop is `border` and the source is not read */

/* One frame's parameters.  Plain data, 72 bytes, no padding, 8-byte aligned. */
typedef struct dfd_align_frame {
  int64_t q[6];         /* inverse map canvas -> full frame in Q16, q = rint(A * 65536): x = (q0 X + q1 Y + q2) / 65536, y from q3..q5 */
  int32_t x0, y0;       /* crop origin on the canvas: output pixel (i, j) is canvas pixel (X, Y) = (x0 + j, y0 + i) */
  int32_t win_x, win_y; /* where the buffer's window starts in full-frame coordinates (0, 0 for a whole frame) */
  int32_t border;       /* value of every tap outside the window; clamped to 0..255 */
  uint32_t flags;       /* DFD_ALIGN_FRAME_*; other bits 0 */
} dfd_align_frame_t;

#define DFD_ALIGN_FRAME_BYTES 72

/* out[f] = the out_h x out_w cut at (x0, y0) of frame f warped onto the canvas, bilinear, constant border.
 *   in            u8 on the device: n_frames windows of win_h x win_w pixels, frame f at in + f * frame_stride, row r of a
 *                 plane at + r * row_stride (bytes; padding allowed; row_stride >= 3 * win_w interleaved, >= win_w planar;
 *                 frame_stride >= the bytes one frame spans).  The last frame ends with the last pixel of its last row:
 *                 nothing behind it is read, and no row padding is ever read.
 *   out           u8 planar [n_frames, 3, out_h, out_w], dense; must not overlap `in`
 *   frames        dfd_align_frame_t [n_frames] on the device, 8-byte aligned
 * Arithmetic, all integer (two's complement, 64-bit, wrapping), for output pixel (i, j) of a frame:
 *   X = x0 + j, Y = y0 + i;  xf = q0 X + q1 Y + q2,  yf = q3 X + q4 Y + q5
 *   x5 = (xf + 1024) >> 11 (arithmetic shift), sx = x5 >> 5, fx = x5 & 31; y5, sy, fy likewise from yf
 *   taps (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1) with weights (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx fy (sum 1024)
 *   out = (sum of weight * tap + 512) >> 10
 * A tap whose full-frame position lies outside [win_y, win_y + win_h) x [win_x, win_x + win_w) counts as `border` and is not
 * loaded, so no record can make the kernel read outside the buffer; positions far outside give `border`, they do not wrap
 * (|q| < 2^40 with |x0|, |y0| < 2^20 cannot overflow 64 bits).  One launch, no workspace, no atomics; every byte of `out`
 * is written exactly once.  n_frames == 0 is a successful no-op. */
int dfd_align_crop_u8(const uint8_t* in, int layout, int64_t row_stride, int64_t frame_stride, int win_h, int win_w, uint8_t* out,
                      int n_frames, int out_h, int out_w, const dfd_align_frame_t* frames, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_ALIGN_H */
