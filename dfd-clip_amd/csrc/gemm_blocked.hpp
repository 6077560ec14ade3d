// The fragment-blocked layout of the MLP intermediate `u` (c_fc's output, c_proj's A operand) — THE definition, included
// by the epilogue that writes it (gemm256p_common.hpp, tile_epilogue) and by the loader that reads it (gemm256e.hip,
// set_a); dfd-clip_amd/blocked.py restates it for tests and for anything else that must look at `u`.
//
// A matrix [M, C] of bf16 with leading dimension ld (ld % 64 == 0) keeps its footprint — row groups of 16 rows, 32 ld
// bytes apiece, rows rounded up to 16 — but inside a row group the bytes are ordered
//     [kt = 0 .. C/64)[s = 0..1][er = 0..15][eq = 0..3][16 B]
// One (row group, kt) block of 2 KB is a UNIT: 16 rows of one 64-channel K tile of c_proj.  The 16-byte piece (s, er, eq)
// holds channels 64 kt + 16 eq + 8 s .. + 7 of row 16 g + er, i.e. 16-byte chunk c = 2 eq + s of the row's 128 bytes of
// that K tile.  Row-group-major, K tile minor: a wave of c_proj walks ONE row group along K, so its unit loads are one
// run of 2 (C/64) KB, as its row loads were runs of 2 C bytes.
//   * c_fc's accumulator fragment of lane (er, eq), once the output channels are permuted (below), is the 32 bytes
//     (s = 0, 1) of row er at eq: a wave store of one s writes 1 KB of contiguous memory, no exchange between lanes.
//   * c_proj's LDS-DMA piece of 8 rows x 8 chunks reads two runs of 512 bytes (s = 0: er 0..7 or 8..15, every eq; s = 1).
// Rows >= M of the last group are never written and never read.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DFD_BLK_FN __host__ __device__ __forceinline__
#else
#define DFD_BLK_FN inline
#endif

constexpr uint32_t DFD_BLK_UNIT = 2048;  // bytes of a unit = the K-tile step inside a row group

// byte offset of row r (its group + its 64-byte line inside a half unit); ld_bytes = bytes of a row-major row
DFD_BLK_FN uint32_t dfd_blk_row(uint32_t r, uint32_t ld_bytes) { return (r >> 4) * (ld_bytes * 16u) + (r & 15u) * 64u; }
// ... of 16-byte chunk c (0..7) of a K tile: s = c & 1 selects the half unit, eq = c >> 1 the piece of the row's line
DFD_BLK_FN uint32_t dfd_blk_chunk(uint32_t c) { return (c & 1u) * 1024u + (c >> 1) * 16u; }

// Channel permutation of the GEMM that WRITES the layout, inside every aligned group of 64 output channels: MFMA column
// c = 16 j + 4 eq + e (accumulator fragment j, lane quarter eq, element e) computes true channel 16 eq + 4 j + e, so
// that a lane's acc[i][0..3] are 16 consecutive channels of its row.  (Swaps two 2-bit fields: its own inverse.)  The
// host applies it to the rows of the weight and to the bias once; every channel's dot product is unchanged.
DFD_BLK_FN uint32_t dfd_blk_true_channel(uint32_t c) { return (c & ~60u) | ((c & 12u) << 2) | ((c & 48u) >> 2); }
