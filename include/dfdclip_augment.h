/* dfdclip_augment.h — device-side training augmentation of libdfdclip_hip.so: the colour, JPEG and flip transforms of the
 * reference's `normal` and `frame` presets (src/datasets.py:288-399) on uint8 frames that are already on the device.  Added
 * beside the C ABI of dfdclip.h WITHOUT a new DFD_ABI_VERSION (still 17): nothing in dfdclip.h, dfdclip_ext.h or
 * dfdclip_explain.h changed.  A library built before it lacks the symbol, which the loader reports by name.  Conventions
 * (device pointers, `stream`, return codes, dfd_last_error) are dfdclip.h's.
 *
 * It lives in a header of its own because the function lists of the other headers are pinned by their tests.  The Python
 * binding lists it in capi.AUGMENT_SIGNATURES; tests/test_augment_cpu.py checks header, table and struct size against each
 * other, tests/test_hip_augment.py the kernel against the integer restatement in dfd-clip_amd/augment.py, bit for bit. */
#ifndef DFDCLIP_AUGMENT_H
#define DFDCLIP_AUGMENT_H

#include <stdint.h>

#include "dfdclip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFD_AUG_RGB_LUT 1u  /* rgb_lut[c][v] replaces v in channel c */
#define DFD_AUG_HSV 2u      /* hue / sat / val are added on OpenCV's 8-bit HSV scales */
#define DFD_AUG_TONE_LUT 4u /* tone_lut[v] replaces v in every channel */
#define DFD_AUG_FLIP 8u     /* columns are mirrored on the store */

/* One parameter set: what one draw of the reference's Compose applies to a frame.  Frames of one clip share a set
 * (sequence augmentation); per-frame augmentation gives each frame its own.  Plain data, 1056 bytes, no padding. */
typedef struct dfd_augment_set {
  uint32_t flags;         /* DFD_AUG_* */
  int32_t hue, sat, val;  /* hue is added mod 180 (H in [0,180)); sat and val are added with saturation to [0,255] (any int32) */
  int32_t quality;        /* JPEG quality 1..100; 0 = no compression; values above 100 count as 100, below 0 as 0 */
  int32_t reserved[3];    /* 0 */
  uint8_t rgb_lut[3][256];
  uint8_t tone_lut[256];
} dfd_augment_set_t;

#define DFD_AUGMENT_SET_BYTES 1056

/* out[f] = flip(jpeg(tone(hsv(rgb_lut(in[f]))))) with the set sets[set_of_frame[f]], stage by stage in that order; each
 * stage runs only when its flag (or a quality > 0) asks for it.  A frame whose index lies outside [0, n_sets) is copied.
 *   in, out        u8 planar [n_frames, 3, h, w], dense; they must not overlap (in == out is refused)
 *   sets           dfd_augment_set_t [n_sets] on the device; n_sets >= 1 when n_frames > 0
 *   set_of_frame   i32 [n_frames] on the device
 * All arithmetic is integer: the HSV stage uses round-to-nearest integer divisions, the JPEG stage libjpeg's baseline
 * pipeline (RGB->YCbCr, 4:2:0 by 2x2 averaging, slow-integer 8x8 DCT, Annex-K tables scaled by quality, quantise,
 * dequantise, inverse DCT, triangle chroma upsampling, YCbCr->RGB) in int32 fixed point, with frames padded by edge
 * replication to whole 16x16 MCUs.  One launch, no workspace, no atomics; every byte of `out` is written exactly once. */
int dfd_augment_u8(const uint8_t* in, uint8_t* out, int n_frames, int h, int w, const dfd_augment_set_t* sets, int n_sets,
                   const int32_t* set_of_frame, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_AUGMENT_H */
