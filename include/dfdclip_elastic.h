/* dfdclip_elastic.h — device-side elastic warp of libdfdclip_hip.so: the transform behind the reference's self-supervised
 * fakes (`ssl_fake`, src/datasets.py:401-418, :538-544, :667-669: one `alb.ElasticTransform(alpha=50, sigma=6,
 * alpha_affine=0, p=1)` draw replayed over every frame of a real clip, which is then labelled fake), on uint8 clips that are
 * already on the device.  Added beside the C ABI of dfdclip.h WITHOUT a new DFD_ABI_VERSION (still 17): nothing in dfdclip.h,
 * dfdclip_ext.h, dfdclip_explain.h, dfdclip_augment.h or dfdclip_align.h changed.  A library built before it lacks the
 * symbols, which the loader reports by name.  Conventions (device pointers, `stream`, return codes, dfd_last_error) are
 * dfdclip.h's.
 *
 * It lives in a header of its own because the function lists of the other headers are pinned by their tests.  The Python
 * binding lists it in capi.ELASTIC_SIGNATURES; tests/test_elastic_cpu.py checks header and table against each other and the
 * integer restatement in dfd-clip_amd/elastic.py against scipy, tests/test_hip_elastic.py the kernels against the
 * restatement, bit for bit.
 *
 * NOT pinned: the pixel values of albumentations / cv2.remap.  The structure is that of albumentations' non-approximate
 * path as it is understood (uniform noise in [-1, 1), scipy's gaussian_filter with boundary `reflect`, times alpha;
 * bilinear sampling with BORDER_REFLECT_101), but neither library is a dependency and the reference holds no fixture, so
 * nothing here checks their bits. */
#ifndef DFDCLIP_ELASTIC_H
#define DFDCLIP_ELASTIC_H

#include <stdint.h>

#include "dfdclip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFD_ELASTIC_MAX_RADIUS 128      /* the blur has at most 2 * 128 + 1 taps */
#define DFD_ELASTIC_TAP_ONE 32768       /* the taps are Q15 and sum to exactly this */
#define DFD_ELASTIC_SITE 0xE1A57100u    /* xor-ed into the low key word: keeps these draws apart from the dropout sites' */
#define DFD_ELASTIC_MAX_SIDE (1 << 24)  /* h and w may not exceed this (and h * w < 2^31) */

/* field[f] = the displacement field with the 64-bit id field_ids[f]: per pixel (dx5, dy5) in 1/32-pixel units.
 *   field       i16 [n_fields, h, w, 2] on the device (dx5 first), 4-byte aligned: the caller's workspace of
 *               n_fields * h * w * 4 bytes
 *   field_ids   i64 [n_fields] on the device, 8-byte aligned
 *   taps        i32 [2 * radius + 1] ON THE HOST (copied into the launch): Q15, each >= 0, summing to 32768; 0 <= radius <= 128
 * Arithmetic, all integer (two's complement; arithmetic shifts).  Noise of component c (0: dx, 1: dy) at (y, x): element
 * e = (c * h + y) * w + x takes the 16-bit draw (e & 7) of the Philox4x32-10 block with counter (g_lo, g_hi, id_lo, id_hi),
 * g = e >> 3, and key (seed_lo ^ DFD_ELASTIC_SITE, seed_hi) -- the block layout of the dropout masks: word d >> 1, low half
 * first -- and n = draw - 32768.  With q the taps and r(i, n) = the `reflect` boundary (d c b a | a b c d | d c b a:
 * m = i mod 2n, m < n ? m : 2n - 1 - m, any distance, so h or w may be smaller than the radius):
 *   hor(c, y, x) = (sum_k q[k] * n(c, y, r(x + k - radius, w)) + 2^14) >> 15          |sum| <= 2^30: int32
 *   ver(c, y, x) = sum_k q[k] * hor(c, r(y + k - radius, h), x)                       |ver| <= 2^30: int32
 *   d5 = (ver * alpha_q + 2^32) >> 33 in int64, saturated to int16;  alpha_q = round(256 * alpha)
 * so d5 / 32 = alpha * (the blurred noise of [-1, 1)).  A field depends on (seed, id, h, w, taps, alpha_q) only, never on
 * its position f: replaying an id on another launch or batch gives the same field.  One launch, no atomics; every byte of
 * `field` is written exactly once.  n_fields == 0 is a successful no-op. */
int dfd_elastic_field(int16_t* field, int n_fields, int h, int w, const int64_t* field_ids, uint64_t seed, const int32_t* taps,
                      int radius, int32_t alpha_q, void* stream);

/* out[b, t, c] = in[b, t, c] sampled bilinearly at (x + dx5 / 32, y + dy5 / 32) of field[field_of_clip[b]], for every frame t
 * and channel c of clip b; a clip whose index lies outside [0, n_fields) is copied.
 *   in, out         u8 planar [n_clips, n_frames, 3, h, w], dense; they must not overlap (refused)
 *   field           as dfd_elastic_field wrote it; may be null when n_fields == 0
 *   field_of_clip   i32 [n_clips] on the device
 * Arithmetic, all integer, that of dfd_align_crop_u8: X5 = 32 x + dx5, sx = X5 >> 5, fx = X5 & 31 (Y5, sy, fy likewise); taps
 * (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1) with weights (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx fy (sum 1024);
 * out = (sum of weight * tap + 512) >> 10.  A tap index i outside the frame is brought inside by `reflect_101`
 * (d c b | a b c d | c b a: m = i mod (2n - 2), m < n ? m : 2n - 2 - m; n == 1 maps to 0), valid for any distance, so no
 * field can make the kernel read outside the buffer.  One launch, no workspace, no atomics; every byte of `out` is written
 * exactly once.  n_clips == 0 or n_frames == 0 is a successful no-op. */
int dfd_elastic_remap_u8(const uint8_t* in, uint8_t* out, int n_clips, int n_frames, int h, int w, const int16_t* field, int n_fields,
                         const int32_t* field_of_clip, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_ELASTIC_H */
