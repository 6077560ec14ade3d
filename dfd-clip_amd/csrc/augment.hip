// Device-side training augmentation of uint8 frames: the colour, JPEG and flip transforms of the reference's `normal`
// and `frame` presets (src/datasets.py:288-399: albumentations RGBShift, HueSaturationValue, RandomBrightnessContrast,
// ImageCompression, HorizontalFlip), which the reference runs per frame on the host before `Detector._transform`.
// One launch, one pass: every input byte is read once (plus the halo and the replicated edge, through L2), every
// output byte is written once; no workspace, no atomics.
//
// Arithmetic (restated in dfd-clip_amd/augment.py: augment_reference, which the tests compare with bit for bit).
// Everything is integer, so that the restatement can be exact:
//   rgb lut  : v <- rgb_lut[c][v]
//   hsv      : OpenCV's 8-bit scales.  V = max, d = max - min, S = (255 d + V/2) / V, H = (30 (g - b) [+ 60 d | 120 d]
//              + d/2) / d mod 180 by the channel that holds the max (r, then g, then b); grey: H = S = 0.  H += hue mod
//              180, S and V add with saturation.  Back: sector = H / 30, f = H - 30 sector, p = (V (255 - S) + 127) / 255,
//              q = (V (7650 - S f) + 3825) / 7650, t = (V (7650 - S (30 - f)) + 3825) / 7650.
//   tone lut : v <- tone_lut[v]
//   jpeg     : libjpeg's baseline pipeline in its own fixed point: RGB -> YCbCr with 16-bit constants, 4:2:0 by 2x2
//              averaging with the alternating 1, 2 bias, level shift, slow-integer forward DCT (13-bit constants, 2 pass-1
//              bits), Annex-K tables scaled by quality, quantisation with rounding half away from zero, dequantisation,
//              slow-integer inverse DCT, clamp, triangle ("fancy") upsampling with the chroma plane's own edges
//              replicated, YCbCr -> RGB with 16-bit constants, clamp.  Frames are padded to whole 16x16 MCUs as libjpeg
//              pads them: luma and the chroma source by replicating the last column / row of the input, chroma rows
//              beyond the last real chroma row by replicating that row.
//   flip     : column x goes to w - 1 - x on the store.
//
// A 256-thread workgroup owns a 64x64 tile (4x4 MCUs) of one frame.  Triangle upsampling reads one chroma sample beyond
// each tile edge, which costs that neighbour's whole 8x8 chroma block, so a JPEG tile stages up to 96x96 pixels (the tile
// and a ring of MCUs, where the frame has them) and transforms chroma for the ring as well: 64 luma + 2 * 36 chroma
// blocks for 64 * 64 pixels instead of 64 + 2 * 16.  The colour stages run on the way into LDS, 4 pixels per thread with
// one (unaligned-capable) dword load per channel.  The DCTs run 32 blocks at a time, one thread per block row or column:
// pass 1 writes its row transposed into a [32][72]-dword buffer (the stride 72 keeps both the dword stores of 8 blocks
// and the 32-byte reads of a column conflict-free), the column thread finishes the forward DCT, quantises, dequantises
// and runs the inverse DCT's column pass in registers, and the row thread of the last pass writes u8 samples into the
// planes the store phase upsamples from.  Divisions by the quantiser are one multiply-high each (FastDiv constants built
// once per workgroup).  LDS: 27 KiB staged RGB + 9 KiB DCT buffer + 8.5 KiB decoded planes + 2.5 KiB tables.
#include "common.hpp"
#include "../../include/dfdclip_augment.h"

namespace {

constexpr int TILE = 64;             // output pixels per workgroup side: 4 MCUs
constexpr int MCU = 16;
constexpr int REG = TILE + 2 * MCU;  // staged side with the ring
constexpr int SLOTS = 32;            // 8x8 blocks transformed per round: 256 threads / 8
constexpr int WSTRIDE = 72;          // dwords per block in the DCT buffer (64 + 8)
constexpr int CPITCH = REG / 2;      // decoded chroma plane pitch

struct AugArgs {
  const uint8_t* in;
  uint8_t* out;
  const dfd_augment_set_t* sets;
  const int32_t* set_of_frame;
  int n_frames, h, w, n_sets;
  int tiles_x, tiles_y;
};

__constant__ uint8_t k_quant_base[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// libjpeg's slow-integer DCT constants: FIX(x) = round(x * 2^13)
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
              F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
              F_2_562915447 = 20995, F_3_072711026 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One 8-point forward DCT in place; FIRST: the row pass (results scaled up by 2^PASS1_BITS), else the column pass.
template <bool FIRST>
__device__ __forceinline__ void fdct8(int* d) {
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int SH = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
  if (FIRST) {
    d[0] = (tmp10 + tmp11) << PASS1_BITS;
    d[4] = (tmp10 - tmp11) << PASS1_BITS;
  } else {
    d[0] = descale(tmp10 + tmp11, PASS1_BITS);
    d[4] = descale(tmp10 - tmp11, PASS1_BITS);
  }
  int z1 = (tmp12 + tmp13) * F_0_541196100;
  d[2] = descale(z1 + tmp13 * F_0_765366865, SH);
  d[6] = descale(z1 - tmp12 * F_1_847759065, SH);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * F_1_175875602;
  const int t4 = tmp4 * F_0_298631336, t5 = tmp5 * F_2_053119869, t6 = tmp6 * F_3_072711026, t7 = tmp7 * F_1_501321110;
  z1 *= -F_0_899976223;
  z2 *= -F_2_562915447;
  z3 = z3 * -F_1_961570560 + z5;
  z4 = z4 * -F_0_390180644 + z5;
  d[7] = descale(t4 + z1 + z3, SH);
  d[5] = descale(t5 + z2 + z4, SH);
  d[3] = descale(t6 + z2 + z3, SH);
  d[1] = descale(t7 + z1 + z4, SH);
}

// One 8-point inverse DCT in place; FIRST: the column pass, else the row pass (which leaves level-shifted samples).
template <bool FIRST>
__device__ __forceinline__ void idct8(int* d) {
  constexpr int SH = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS + 3;
  int z2 = d[2], z3 = d[6];
  int z1 = (z2 + z3) * F_0_541196100;
  int tmp2 = z1 - z3 * F_1_847759065;
  int tmp3 = z1 + z2 * F_0_765366865;
  int tmp0 = (d[0] + d[4]) << CONST_BITS;
  int tmp1 = (d[0] - d[4]) << CONST_BITS;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = d[7];
  tmp1 = d[5];
  tmp2 = d[3];
  tmp3 = d[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * F_1_175875602;
  tmp0 *= F_0_298631336;
  tmp1 *= F_2_053119869;
  tmp2 *= F_3_072711026;
  tmp3 *= F_1_501321110;
  z1 *= -F_0_899976223;
  z2 *= -F_2_562915447;
  z3 = z3 * -F_1_961570560 + z5;
  z4 = z4 * -F_0_390180644 + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  d[0] = descale(tmp10 + tmp3, SH);
  d[7] = descale(tmp10 - tmp3, SH);
  d[1] = descale(tmp11 + tmp2, SH);
  d[6] = descale(tmp11 - tmp2, SH);
  d[2] = descale(tmp12 + tmp1, SH);
  d[5] = descale(tmp12 - tmp1, SH);
  d[3] = descale(tmp13 + tmp0, SH);
  d[4] = descale(tmp13 - tmp0, SH);
}

// libjpeg's colour constants: FIX(x) = round(x * 2^16)
__device__ __forceinline__ int to_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int to_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int to_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

__device__ __forceinline__ void hsv_shift(int& r, int& g, int& b, int hue, int sat, int val) {
  int v = max(r, max(g, b));
  const int d = v - min(r, min(g, b));
  int s = v ? (d * 255 + (v >> 1)) / v : 0;
  int hh = 0;
  if (d) {
    int num = v == r ? (g - b) * 30 : (v == g ? (b - r) * 30 + 60 * d : (r - g) * 30 + 120 * d);
    if (num < 0) num += 180 * d;
    hh = (num + (d >> 1)) / d;
    if (hh >= 180) hh -= 180;
  }
  hh += hue;  // hue already in [0, 180)
  if (hh >= 180) hh -= 180;
  s = clamp255(s + sat);
  v = clamp255(v + val);
  const int sector = hh / 30, f = hh - 30 * sector;
  const int p = (v * (255 - s) + 127) / 255;
  const int q = (v * (7650 - s * f) + 3825) / 7650;
  const int t = (v * (7650 - s * (30 - f)) + 3825) / 7650;
  switch (sector) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

__device__ __forceinline__ uint32_t load_u32(const uint8_t* p) {  // any alignment: one global_load_dword
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
__device__ __forceinline__ void store_u32(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

__global__ __launch_bounds__(256) void augment_u8_kernel(AugArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_rgb[3][REG][REG];
  __shared__ __attribute__((aligned(16))) int s_w[SLOTS * WSTRIDE];
  __shared__ __attribute__((aligned(16))) uint8_t s_y[TILE][TILE];
  __shared__ __attribute__((aligned(16))) uint8_t s_c[2][CPITCH][CPITCH];
  __shared__ __attribute__((aligned(16))) uint8_t s_lut[4][256];
  __shared__ int s_q[2][64];
  __shared__ uint32_t s_qmul[2][64], s_qsh[2][64];

  const int tid = threadIdx.x;
  const int h = a.h, w = a.w;
  const int tx = blockIdx.x % a.tiles_x;
  const int ty = (blockIdx.x / a.tiles_x) % a.tiles_y;
  const int n = blockIdx.x / (a.tiles_x * a.tiles_y);
  const int64_t plane = (int64_t)h * w;
  const uint8_t* src = a.in + (int64_t)n * 3 * plane;
  uint8_t* dst = a.out + (int64_t)n * 3 * plane;
  const int X0 = tx * TILE, Y0 = ty * TILE;
  const int X1 = min(X0 + TILE, w), Y1 = min(Y0 + TILE, h);

  const int si = a.set_of_frame[n];
  const bool have = si >= 0 && si < a.n_sets;
  const dfd_augment_set_t* set = a.sets + (have ? si : 0);
  uint32_t flags = 0;
  int hue = 0, sat = 0, val = 0, quality = 0;
  if (have) {
    flags = set->flags & (DFD_AUG_RGB_LUT | DFD_AUG_HSV | DFD_AUG_TONE_LUT | DFD_AUG_FLIP);
    hue = (set->hue % 180 + 180) % 180;
    sat = min(max(set->sat, -255), 255);  // beyond +-255 the saturating add gives the same; no overflow in s + sat
    val = min(max(set->val, -255), 255);
    quality = min(max(set->quality, 0), 100);
  }

  if (flags == 0 && quality == 0) {  // copy: this tile's rows, dword by dword
    const int ng = (X1 - X0 + 3) >> 2, rows = Y1 - Y0;
    for (int e = tid; e < 3 * rows * ng; e += 256) {
      const int g = e % ng, cy = e / ng;
      const int c = cy / rows, yy = cy - c * rows;
      const int64_t off = c * plane + (int64_t)(Y0 + yy) * w + X0 + 4 * g;
      if (X0 + 4 * g + 4 <= w) {
        store_u32(dst + off, load_u32(src + off));
      } else {
        for (int k = 0; X0 + 4 * g + k < w; ++k) dst[off + k] = src[off + k];
      }
    }
    return;
  }

  if (flags & (DFD_AUG_RGB_LUT | DFD_AUG_TONE_LUT))  // rgb_lut and tone_lut are contiguous: 256 dwords
    reinterpret_cast<uint32_t*>(&s_lut[0][0])[tid] = reinterpret_cast<const uint32_t*>(&set->rgb_lut[0][0])[tid];
  if (quality > 0 && tid < 128) {
    const int t = tid >> 6, i = tid & 63;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = min(max(((int)k_quant_base[t][i] * scale + 50) / 100, 1), 255);
    const uint32_t d = 8u * q;  // the slow-integer DCT leaves its output scaled by 8
    uint32_t s = 3;
    while ((1u << s) < d) ++s;
    s_q[t][i] = q;
    s_qmul[t][i] = (uint32_t)(((1ull << (31 + s)) + d - 1) / d);  // floor(x / d) = umulhi(x, mul) >> (s - 1), x < 2^31
    s_qsh[t][i] = s - 1;
  }

  // staged region: the tile, and for JPEG a ring of MCUs where the padded frame has them
  const int pw = (w + MCU - 1) & ~(MCU - 1), ph = (h + MCU - 1) & ~(MCU - 1);
  int rx0 = X0, ry0 = Y0, rw = (X1 - X0 + 3) & ~3, rh = Y1 - Y0;
  if (quality > 0) {
    rx0 = max(X0 - MCU, 0);
    ry0 = max(Y0 - MCU, 0);
    rw = min(X0 + TILE + MCU, pw) - rx0;
    rh = min(Y0 + TILE + MCU, ph) - ry0;
  }
  const int ox = X0 - rx0, oy = Y0 - ry0;
  __syncthreads();

  {  // load with edge replication; colour stages on the way
    const int rq = rw >> 2;
    for (int e = tid; e < rh * rq; e += 256) {
      const int i = e / rq, q4 = e - i * rq;
      const int x = rx0 + 4 * q4;
      const uint8_t* p = src + (int64_t)min(ry0 + i, h - 1) * w;
      uint32_t c4[3];
      if (x + 4 <= w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) c4[c] = load_u32(p + c * plane + x);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          c4[c] = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) c4[c] |= (uint32_t)p[c * plane + min(x + k, w - 1)] << (8 * k);
        }
      }
      if (flags & (DFD_AUG_RGB_LUT | DFD_AUG_HSV | DFD_AUG_TONE_LUT)) {
        uint32_t o4[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          int r = (c4[0] >> (8 * k)) & 255, g = (c4[1] >> (8 * k)) & 255, b = (c4[2] >> (8 * k)) & 255;
          if (flags & DFD_AUG_RGB_LUT) {
            r = s_lut[0][r];
            g = s_lut[1][g];
            b = s_lut[2][b];
          }
          if (flags & DFD_AUG_HSV) hsv_shift(r, g, b, hue, sat, val);
          if (flags & DFD_AUG_TONE_LUT) {
            r = s_lut[3][r];
            g = s_lut[3][g];
            b = s_lut[3][b];
          }
          o4[0] |= (uint32_t)r << (8 * k);
          o4[1] |= (uint32_t)g << (8 * k);
          o4[2] |= (uint32_t)b << (8 * k);
        }
        c4[0] = o4[0];
        c4[1] = o4[1];
        c4[2] = o4[2];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(&s_rgb[c][i][4 * q4]) = c4[c];
    }
  }
  __syncthreads();

  const int ch = (h + 1) >> 1, cw = (w + 1) >> 1;  // real chroma plane
  if (quality > 0) {
    const int lbx = (min(X0 + TILE, pw) - X0) >> 3, lby = (min(Y0 + TILE, ph) - Y0) >> 3;  // luma blocks of the tile
    const int rmx = rw >> 4, rmy = rh >> 4;                                                // MCUs of the region
    const int L = lbx * lby, C = rmx * rmy, NB = L + 2 * C;
    const int slot = tid >> 3, r = tid & 7;
    int* wb = s_w + slot * WSTRIDE;
    for (int base = 0; base < NB; base += SLOTS) {
      const int id = base + slot;
      const bool on = id < NB;
      int comp = 0, bx = 0, by = 0;  // 0 luma (block of the tile), 1 cb, 2 cr (block of the region)
      if (id < L) {
        by = id / lbx;
        bx = id - by * lbx;
      } else {
        int j = id - L;
        comp = 1;
        if (j >= C) {
          j -= C;
          comp = 2;
        }
        by = j / rmx;
        bx = j - by * rmx;
      }
      int d[8];
      if (on) {  // pass A: samples of row r, forward row pass, transposed store
        if (comp == 0) {
          const int i = oy + 8 * by + r, j0 = ox + 8 * bx;
          uint32_t c4[3][2];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            c4[c][0] = *reinterpret_cast<const uint32_t*>(&s_rgb[c][i][j0]);
            c4[c][1] = *reinterpret_cast<const uint32_t*>(&s_rgb[c][i][j0 + 4]);
          }
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int sh = 8 * (k & 3);
            d[k] = to_luma((c4[0][k >> 2] >> sh) & 255, (c4[1][k >> 2] >> sh) & 255, (c4[2][k >> 2] >> sh) & 255) - 128;
          }
        } else {
          // chroma rows past the plane's last real row repeat that row (libjpeg pads the downsampled plane)
          const int cy = min((ry0 >> 1) + 8 * by + r, ch - 1);
          const int i0 = 2 * cy - ry0, j0 = 16 * bx;
#pragma unroll
          for (int k4 = 0; k4 < 4; ++k4) {  // 4 pixels of two rows = 2 chroma samples per step
            uint32_t c4[3][2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              c4[c][0] = *reinterpret_cast<const uint32_t*>(&s_rgb[c][i0][j0 + 4 * k4]);
              c4[c][1] = *reinterpret_cast<const uint32_t*>(&s_rgb[c][i0 + 1][j0 + 4 * k4]);
            }
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
              int sum = 0;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int sh = 8 * (2 * k2 + (e & 1));
                const int R = (c4[0][e >> 1] >> sh) & 255, G = (c4[1][e >> 1] >> sh) & 255, B = (c4[2][e >> 1] >> sh) & 255;
                sum += comp == 1 ? to_cb(R, G, B) : to_cr(R, G, B);
              }
              d[2 * k4 + k2] = ((sum + 1 + k2) >> 2) - 128;
            }
          }
        }
        fdct8<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) wb[k * 8 + r] = d[k];
      }
      __syncthreads();
      if (on) {  // pass B: column r: forward column pass, quantise, dequantise, inverse column pass
        const int4 lo = *reinterpret_cast<const int4*>(wb + r * 8), hi = *reinterpret_cast<const int4*>(wb + r * 8 + 4);
        d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w;
        d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
        fdct8<false>(d);
        const int t = comp ? 1 : 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int q = s_q[t][j * 8 + r];
          const int v = d[j];
          const uint32_t mag = (uint32_t)(v < 0 ? -v : v) + 4u * q;
          const int lev = (int)(__umulhi(mag, s_qmul[t][j * 8 + r]) >> s_qsh[t][j * 8 + r]);
          d[j] = (v < 0 ? -lev : lev) * q;
        }
        idct8<true>(d);
      }
      __syncthreads();
      if (on) {
#pragma unroll
        for (int j = 0; j < 8; ++j) wb[j * 8 + r] = d[j];
      }
      __syncthreads();
      if (on) {  // pass C: row r: inverse row pass, samples
        const int4 lo = *reinterpret_cast<const int4*>(wb + r * 8), hi = *reinterpret_cast<const int4*>(wb + r * 8 + 4);
        d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w;
        d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
        idct8<false>(d);
        uint2 px = {0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          px.x |= (uint32_t)clamp255(d[k] + 128) << (8 * k);
          px.y |= (uint32_t)clamp255(d[k + 4] + 128) << (8 * k);
        }
        uint8_t* o = comp == 0 ? &s_y[8 * by + r][8 * bx] : &s_c[comp - 1][8 * by + r][8 * bx];
        *reinterpret_cast<uint2*>(o) = px;
      }
      __syncthreads();
    }
  }

  {  // store: 4 output pixels per thread, mirrored columns when asked
    const bool flip = flags & DFD_AUG_FLIP;
    const int ow = X1 - X0, ng = (ow + 3) >> 2, rows = Y1 - Y0;
    const int O0 = flip ? w - X1 : X0;
    const int cy0 = ry0 >> 1, cx0 = rx0 >> 1;
    for (int e = tid; e < rows * ng; e += 256) {
      const int yy = e / ng, g = e - yy * ng;
      const int y = Y0 + yy;
      const int nv = min(4, ow - 4 * g);
      uint32_t o4[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nv) {
          const int xo = O0 + 4 * g + k;
          const int x = flip ? w - 1 - xo : xo;
          const int xx = x - X0;
          int R, G, B;
          if (quality > 0) {
            const int cy = y >> 1, cx = x >> 1;
            const int ny = ((y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0)) - cy0;
            const int nx = ((x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0)) - cx0;
            const int bias = (x & 1) ? 7 : 8;
            int cc[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const int here = 3 * s_c[c][cy - cy0][cx - cx0] + s_c[c][ny][cx - cx0];
              const int next = 3 * s_c[c][cy - cy0][nx] + s_c[c][ny][nx];
              cc[c] = ((3 * here + next + bias) >> 4) - 128;
            }
            const int Y = s_y[yy][xx];
            R = clamp255(Y + ((91881 * cc[1] + 32768) >> 16));
            G = clamp255(Y + ((-22554 * cc[0] - 46802 * cc[1] + 32768) >> 16));
            B = clamp255(Y + ((116130 * cc[0] + 32768) >> 16));
          } else {
            R = s_rgb[0][yy][xx];
            G = s_rgb[1][yy][xx];
            B = s_rgb[2][yy][xx];
          }
          o4[0] |= (uint32_t)R << (8 * k);
          o4[1] |= (uint32_t)G << (8 * k);
          o4[2] |= (uint32_t)B << (8 * k);
        }
      }
      uint8_t* o = dst + (int64_t)y * w + O0 + 4 * g;
      if (nv == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) store_u32(o + c * plane, o4[c]);
      } else {
        for (int c = 0; c < 3; ++c)
          for (int k = 0; k < nv; ++k) o[c * plane + k] = (uint8_t)(o4[c] >> (8 * k));
      }
    }
  }
}

}  // namespace

extern "C" int dfd_augment_u8(const uint8_t* in, uint8_t* out, int n_frames, int h, int w, const dfd_augment_set_t* sets,
                              int n_sets, const int32_t* set_of_frame, void* stream) {
  static_assert(sizeof(dfd_augment_set_t) == DFD_AUGMENT_SET_BYTES, "dfd_augment_set_t must stay 1056 bytes");
  DFD_REQUIRE(n_frames >= 0 && h > 0 && w > 0 && n_sets >= 0, "dfd_augment_u8: bad shape (n=%d %dx%d, %d sets)", n_frames, h, w, n_sets);
  if (n_frames == 0) return DFD_OK;
  DFD_REQUIRE(in && out && set_of_frame, "dfd_augment_u8: null pointer");
  DFD_REQUIRE(n_sets > 0 && sets, "dfd_augment_u8: %d frames but no parameter set", n_frames);
  const int64_t bytes = (int64_t)n_frames * 3 * h * w;
  DFD_REQUIRE(in + bytes <= out || out + bytes <= in,
              "dfd_augment_u8: in and out overlap; the augmentation is not done in place (tiles read their neighbours)");
  DFD_REQUIRE((reinterpret_cast<uintptr_t>(sets) & 3) == 0 && (reinterpret_cast<uintptr_t>(set_of_frame) & 3) == 0,
              "dfd_augment_u8: sets and set_of_frame must be 4-byte aligned");
  AugArgs a;
  a.in = in;
  a.out = out;
  a.sets = sets;
  a.set_of_frame = set_of_frame;
  a.n_frames = n_frames;
  a.h = h;
  a.w = w;
  a.n_sets = n_sets;
  a.tiles_x = (w + TILE - 1) / TILE;
  a.tiles_y = (h + TILE - 1) / TILE;
  const int64_t blocks = (int64_t)n_frames * a.tiles_x * a.tiles_y;
  DFD_REQUIRE(blocks < (1ll << 31), "dfd_augment_u8: too many tiles (%lld)", (long long)blocks);
  hipLaunchKernelGGL(augment_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  DFD_CHECK_LAUNCH("dfd_augment_u8");
  return DFD_OK;
}
