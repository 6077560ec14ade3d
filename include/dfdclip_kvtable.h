/* dfdclip_kvtable.h — decoder attention over a frame store for libdfdclip_hip.so (dfd_clip_amd/stream.py): the decoder's
 * forward and its attention map read the frames of every clip (= window) out of a store of frames through a slot table, in
 * place, with no copy of the frames in between:
 *   dfd_decoder_attn_fwd_frames    dfd_decoder_attn_fwd  with frame tf of clip b = frame frame_table[b*T + tf] of the store
 *   dfd_decoder_attn_map_frames    dfd_decoder_attn_map  with the same keys
 * Added beside the C ABI of dfdclip.h WITHOUT a new DFD_ABI_VERSION (still 17): no other header changed.  A library built
 * before it lacks the symbols, which the loader reports by name.  Conventions (device pointers, `stream`, return codes,
 * dfd_last_error) are dfdclip.h's.  The Python binding lists the entry points in capi.KVTABLE_SIGNATURES;
 * tests/test_kvtable_cpu.py checks header and table against each other, tests/test_hip_kvtable.py the kernels bit for bit
 * against the untabled entry points run on `stream.table_reference` of the same operands.
 *
 * Addressing.  k (and v) point at the first row of ONE LAYER of the store, not at a clip.  Row p of frame tf of clip b
 * starts at  base + slot*frame_stride + p*row_stride  ELEMENTS, slot = frame_table[b*T + tf], with the strides of `layout`
 * (NULL: rows of heads*64 elements, frames of `patches` rows, as in dfdclip.h).  Every entry of the table is clamped to
 * [0, store_frames) in the kernel before any address is formed, so a bad table reads a wrong frame of the store and never
 * leaves it; the product slot*frame_stride is formed in 64 bits, so a store above 2^31 elements is fine.  Frames may be
 * named any number of times, by one clip or by many.  What stays relative to the clip: frame_mask [B, T] (entry (b, tf)
 * masks the keys of frame tf of clip b, whatever slot they come from) and layout->pos [T, D], whose row tf is added to the
 * rows of frame tf.
 *
 * Arithmetic.  That of the untabled entry points, in the same order: the outputs equal, bit for bit, those of
 * dfd_decoder_attn_fwd / dfd_decoder_attn_map on a dense [B*T, patches, D] copy of the named frames.  The K / V loads are
 * plain whatever dfd_stream_policy_set (dfdclip_hooks.h) says: a stored frame is read by every clip that names it, so it is
 * no read-once stream.  Results do not depend on that. */
#ifndef DFDCLIP_KVTABLE_H
#define DFDCLIP_KVTABLE_H

#include <stdint.h>

#include "dfdclip.h"
#include "dfdclip_explain.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dfd_decoder_attn_fwd (dfdclip.h) over a frame store.  Every argument up to `d` is that entry point's, with k and v as
 * above; the workspace is dfd_decoder_attn_workspace(B, heads, d, splits) bytes, and splits, ext_weights, mix_softmax and
 * stats mean what they mean there.
 *   frame_table   device int32 [B*T]: the store frame of every (clip, frame)
 *   store_frames  frames in one layer of the store (the clamp's range)
 * Nothing outside mix, mix_softmax (when given), stats and the workspace is written; no byte of the store outside the rows
 * of the frames named (after the clamp) is read.  B == 0 is a successful no-op.  Refused with DFD_ERR_INVALID_ARG and a
 * message, without a launch: a null frame_table, store_frames <= 0, and everything dfd_decoder_attn_fwd refuses, in its words
 * under this entry point's name. */
int dfd_decoder_attn_fwd_frames(const float* q, const void* k, const void* v, int kv_dtype, const dfd_kv_layout_t* layout,
                                const uint8_t* frame_mask, const float* ext_weights, float* mix, float* mix_softmax,
                                float* stats, void* workspace, int splits, int B, int T, int patches, int heads, int d,
                                const int32_t* frame_table, int store_frames, void* stream);

/* dfd_decoder_attn_map (dfdclip_explain.h) over a frame store: the per-key weights that dfd_decoder_attn_fwd_frames applied,
 * from the stats it wrote, with the same k, layout, frame_table and store_frames.  Nothing outside aff and branches (when
 * given) is written.  B == 0 is a successful no-op.  Refused as above, and as dfd_decoder_attn_map refuses. */
int dfd_decoder_attn_map_frames(const float* q, const void* k, int kv_dtype, const dfd_kv_layout_t* layout,
                                const uint8_t* frame_mask, const float* stats, const float* ext_weights, float* aff,
                                float* branches, int B, int T, int patches, int heads, int d,
                                const int32_t* frame_table, int store_frames, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFDCLIP_KVTABLE_H */
