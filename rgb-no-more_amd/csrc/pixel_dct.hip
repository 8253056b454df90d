// RGB pixels <-> quantised DCT coefficients in the read_coefficients layout (reference: dct_manip.quantize_at_quality /
// decode_coeff, dct_manip/dct_manip.cpp:315-375, 485-576, which go through IJG libjpeg 9 with 4:2:0 sampling; the users are
// utils/custom_transforms.py:1140-1196, rgb_to_dct / ycbcr_to_rgb).
//
// The unit of work is one 16 x 16 MCU (four luma blocks, one Cb and one Cr block); a grayscale image is cut into groups of four
// consecutive luma blocks instead.  A wave owns a unit, a workgroup of four waves a group of four units, and the workgroups stride
// over the groups, so that a unit count that does not fill the last group (or the grid) is an ordinary path.  Every wave works in
// its own LDS region; the barriers only order a wave's own LDS stores before its lanes read each other's values.
//
// ENCODE.  Luma is 32-bit integer arithmetic throughout and equals libjpeg bit for bit: the fixed-point colour conversion
// (jccolor.c), the "islow" forward DCT (13-bit constants, 2 pass-1 bits; the result is 8 x the DCT) and the quantiser
// sign(c) (|c| + 4 q) / (8 q).  IJG 9 does not average chroma 2 x 2: it takes the 16 x 16-point DCT of the 16 x 16 chroma square and
// keeps the low 8 x 8,  F[u][v] = c(u) c(v) / 16 sum_{m,n<16} (x[m][n] - 128) cos((2m+1) u pi / 32) cos((2n+1) v pi / 32).  Here that
// is two 8 x 16 basis products in fp32 (the basis is computed in double on the host), F / q rounded half away from zero; libjpeg's
// own fixed-point routine differs from the exact value by up to 0.08, so chroma is within 1 of it, not equal.
//
// DECODE.  Dequantise, 8 x 8 inverse DCT for luma, the 8 -> 16 scaled inverse DCT for chroma (IJG 9 up-scales inside the IDCT:
// the transpose of the above with c(u) c(v) / 4), in fp32; each plane sample is floor(x + 0.5) clamped to [0, 255]; then libjpeg's
// fixed-point YCbCr -> RGB (jdcolor.c, 16-bit scale, + ONE_HALF before the shift), clamped.  Where a sample leaves [-128, 383]
// libjpeg's range-limit table wraps; this kernel saturates.
//
// The quantisation tables and the bases travel by value in the kernel arguments (about 1 KB): a call is one launch with no
// allocation, no copy and no synchronisation, and can be captured into a HIP graph.
#include "common.h"
#include "internal.h"
#include "../../include/rgbnm.h"

#include <cmath>

namespace pixdct {

constexpr int WAVES = 4;                 // units per workgroup pass
constexpr int THREADS = 64 * WAVES;
constexpr int MAX_WGS = 2048;            // the grid never exceeds this; further groups are reached by the stride
constexpr int P8 = 9, P16 = 17;          // LDS row pitches of 8- and 16-wide rows (odd: rows fall on different banks)
constexpr int PF = 12;                   // pitch of rows read eight in a row as two 16-byte reads (48 B: aligned, and eight rows apart)

struct EncArgs {
  const uint8_t* px;
  int16_t* Y;
  int16_t* C;
  int H, W, gray, units, nblocks;       // gray: units of four consecutive blocks, nblocks of them in all
  int16_t q[3][64];
  float fb[8][16];                       // fb[u][m] = c(u) / 4 cos((2m+1) u pi / 32)
};

struct DecArgs {
  const int16_t* Y;
  const int16_t* C;
  uint8_t* px;
  int H, W, gray, units, nblocks;
  int16_t q[3][64];
  float ib8[8][8];                       // ib8[u][m]  = c(u) / 2 cos((2m+1) u pi / 16)
  float ib16[8][16];                     // ib16[u][m] = c(u) / 2 cos((2m+1) u pi / 32)
};

// where a colour unit lives: MCU (my, mx) of image b
struct Unit {
  int b, my, mx;
};
__device__ __forceinline__ Unit mcu_of(int unit, int Hm, int Wm) {
  Unit u;
  u.b = unit / (Hm * Wm);
  const int r = unit - u.b * Hm * Wm;
  u.my = r / Wm;
  u.mx = r - u.my * Wm;
  return u;
}

constexpr int FIX16(double x) { return (int)(x * 65536.0 + 0.5); }      // libjpeg's FIX at 16 bits (jccolor.c, jdcolor.c)
// jfdctint.c: FIX at 13 bits
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
              FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
              FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

// one 8-point pass of the islow forward DCT.  PASS 1: input samples - 128, outputs scaled by 4.  PASS 2: outputs descaled by 2 bits
// (0, 4) or 15 bits (the rotations), rounded.
template <int PASS>
__device__ __forceinline__ void fdct8(const int (&d)[8], int (&o)[8]) {
  constexpr int SH = PASS == 1 ? 11 : 15;
  int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
  int t10 = t0 + t3, t12 = t0 - t3, t11 = t1 + t2, t13 = t1 - t2;
  t0 = d[0] - d[7]; t1 = d[1] - d[6]; t2 = d[2] - d[5]; t3 = d[3] - d[4];
  if (PASS == 1) {
    o[0] = (t10 + t11) << 2;
    o[4] = (t10 - t11) << 2;
  } else {
    t10 += 2;
    o[0] = (t10 + t11) >> 2;
    o[4] = (t10 - t11) >> 2;
  }
  int z1 = __mul24(t12 + t13, FIX_0_541196100) + (1 << (SH - 1));
  o[2] = (z1 + __mul24(t12, FIX_0_765366865)) >> SH;
  o[6] = (z1 - __mul24(t13, FIX_1_847759065)) >> SH;
  t12 = t0 + t2;
  t13 = t1 + t3;
  z1 = __mul24(t12 + t13, FIX_1_175875602) + (1 << (SH - 1));
  t12 = __mul24(t12, -FIX_0_390180644) + z1;
  t13 = __mul24(t13, -FIX_1_961570560) + z1;
  z1 = __mul24(t0 + t3, -FIX_0_899976223);
  t0 = __mul24(t0, FIX_1_501321110) + z1 + t12;
  t3 = __mul24(t3, FIX_0_298631336) + z1 + t13;
  z1 = __mul24(t1 + t2, -FIX_2_562915447);
  t1 = __mul24(t1, FIX_3_072711026) + z1 + t13;
  t2 = __mul24(t2, FIX_2_053119869) + z1 + t12;
  o[1] = t0 >> SH;
  o[3] = t1 >> SH;
  o[5] = t2 >> SH;
  o[7] = t3 >> SH;
}

__global__ __launch_bounds__(THREADS) void encode_kernel(EncArgs a) {
  __shared__ int s_q[3][64];
  __shared__ float s_rq[64];                      // 1 / (8 q) of the luma table
  __shared__ __attribute__((aligned(16))) float s_fbT[16][8];      // the basis transposed: [m][u], four u of one m in one read
  __shared__ int s_y[WAVES][4][8][P8];            // luma samples - 128 by block, then the row pass in place
  __shared__ float s_c[WAVES][2][16][16];         // chroma samples - 128
  __shared__ float s_t[WAVES][2][8][P16];         // chroma after the first basis product: [u][n]
  __shared__ __attribute__((aligned(16))) int16_t s_o[WAVES][6][64];

  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  if (tid < 192) s_q[tid >> 6][tid & 63] = a.q[tid >> 6][tid & 63];
  if (tid < 64) s_rq[tid] = 1.0f / (float)(8 * a.q[0][tid]);
  if (tid < 128) s_fbT[tid & 15][tid >> 4] = a.fb[tid >> 4][tid & 15];
  __syncthreads();
  float fbv[16];                                  // the lane's basis row of the second product (v = l % 8), kept in registers
#pragma unroll
  for (int n = 0; n < 16; ++n) fbv[n] = s_fbT[n][l & 7];

  const int H = a.H, W = a.W, Hb = H >> 3, Wb = W >> 3, Hm = H >> 4, Wm = W >> 4;
  const size_t plane = (size_t)H * W;
  const int groups = (a.units + WAVES - 1) / WAVES;
  for (int g = blockIdx.x; g < groups; g += gridDim.x) {
    const int unit = g * WAVES + w;
    const bool live = unit < a.units;            // wave-uniform; a dead wave only keeps the barriers company
    Unit u = {0, 0, 0};
    // ---- load + colour conversion
    if (a.gray) {
      // four consecutive blocks; lane: block l / 16, row (l % 16) / 2, half row l % 2
      const int k = l >> 4, r = (l >> 1) & 7, h4 = (l & 1) * 4;
      const int blk = unit * 4 + k;
      uint32_t v = 0x80808080u;
      if (live && blk < a.nblocks) {
        const int b = blk / (Hb * Wb), rem = blk - b * Hb * Wb, by = rem / Wb, bx = rem - by * Wb;
        v = *reinterpret_cast<const uint32_t*>(a.px + (size_t)b * plane + (size_t)(by * 8 + r) * W + bx * 8 + h4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) s_y[w][k][r][h4 + j] = (int)((v >> (8 * j)) & 255u) - 128;
    } else if (live) {
      u = mcu_of(unit, Hm, Wm);
      const int r = l >> 2, c4 = (l & 3) * 4;
      const uint8_t* p = a.px + (size_t)u.b * 3 * plane + (size_t)(u.my * 16 + r) * W + u.mx * 16 + c4;
      const uint32_t R4 = *reinterpret_cast<const uint32_t*>(p);
      const uint32_t G4 = *reinterpret_cast<const uint32_t*>(p + plane);
      const uint32_t B4 = *reinterpret_cast<const uint32_t*>(p + 2 * plane);
      const int blk = (r >> 3) * 2 + (c4 >> 3), rr = r & 7, cc = c4 & 7;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int R = (R4 >> (8 * j)) & 255, G = (G4 >> (8 * j)) & 255, B = (B4 >> (8 * j)) & 255;
        const int yy = (__mul24(FIX16(0.299), R) + __mul24(FIX16(0.587), G) + __mul24(FIX16(0.114), B) + 32768) >> 16;
        constexpr int OFF = (128 << 16) + 32767;
        const int cb = (__mul24(-FIX16(0.168735892), R) - __mul24(FIX16(0.331264108), G) + __mul24(FIX16(0.5), B) + OFF) >> 16;
        const int cr = (__mul24(FIX16(0.5), R) - __mul24(FIX16(0.418687589), G) - __mul24(FIX16(0.081312411), B) + OFF) >> 16;
        s_y[w][blk][rr][cc + j] = yy - 128;
        s_c[w][0][r][c4 + j] = (float)(cb - 128);
        s_c[w][1][r][c4 + j] = (float)(cr - 128);
      }
    }
    __syncthreads();
    // ---- luma row pass (lanes 0..31: block l / 8, row l % 8), chroma first product (all lanes: four u of one column)
    if (l < 32) {
      int d[8], o[8];
      int* row = s_y[w][l >> 3][l & 7];
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = row[j];
      fdct8<1>(d, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) row[j] = o[j];
    }
    if (!a.gray) {
      const int p = l >> 5, n = l & 15, u0 = ((l >> 4) & 1) * 4;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const float x = s_c[w][p][m][n];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(s_fbT[m][u0 + i], x, acc[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) s_t[w][p][u0 + i][n] = acc[i];
    }
    __syncthreads();
    // ---- luma column pass + quantiser, chroma second product + quantiser
    if (l < 32) {
      const int k = l >> 3, c = l & 7;
      int d[8], o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = s_y[w][k][j][c];
      fdct8<2>(d, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // (|c| + 4 q) / (8 q) without the integer divide: numerator and divisor are below 2^19, so the fp32 product with the
        // rounded reciprocal is within one of the quotient, and the remainder says which way
        const int q8 = 8 * s_q[0][j * 8 + c];
        const int num = (o[j] < 0 ? -o[j] : o[j]) + (q8 >> 1);
        int mag = (int)((float)num * s_rq[j * 8 + c]);
        const int rem = num - __mul24(mag, q8);
        mag += rem >= q8 ? 1 : (rem < 0 ? -1 : 0);
        s_o[w][k][j * 8 + c] = (int16_t)(o[j] < 0 ? -mag : mag);
      }
    }
    if (!a.gray) {
      const int p = l >> 5, v = l & 7, u0 = ((l >> 3) & 3) * 2;
      float acc[2] = {0.f, 0.f};
#pragma unroll
      for (int n = 0; n < 16; ++n) {
        acc[0] = fmaf(s_t[w][p][u0][n], fbv[n], acc[0]);
        acc[1] = fmaf(s_t[w][p][u0 + 1][n], fbv[n], acc[1]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float x = acc[i] / (float)s_q[1][(u0 + i) * 8 + v];
        const float r = floorf(fabsf(x) + 0.5f);
        s_o[w][4 + p][(u0 + i) * 8 + v] = (int16_t)(int)(x < 0.f ? -r : r);
      }
    }
    __syncthreads();
    // ---- finished blocks leave as 16-byte stores: 8 lanes per block
    if (live && l < (a.gray ? 32 : 48)) {
      const int k = l >> 3, part = (l & 7) * 8;
      const int4 val = *reinterpret_cast<const int4*>(&s_o[w][k][part]);
      int16_t* dst = nullptr;
      if (a.gray) {
        const int blk = unit * 4 + k;
        if (blk < a.nblocks) dst = a.Y + (size_t)blk * 64 + part;
      } else if (k < 4) {
        dst = a.Y + (((size_t)u.b * Hb + 2 * u.my + (k >> 1)) * Wb + 2 * u.mx + (k & 1)) * 64 + part;
      } else {
        dst = a.C + ((((size_t)u.b * 2 + (k - 4)) * Hm + u.my) * Wm + u.mx) * 64 + part;
      }
      if (dst) *reinterpret_cast<int4*>(dst) = val;
    }
    // the next pass overwrites s_y / s_c only after its own loads, and every lane that reads s_o has passed the barrier above
    // before any lane can reach the stores into s_o two barriers further on
  }
}

__device__ __forceinline__ int sample_of(float x) {       // floor(x + 0.5) clamped to [0, 255]
  const float r = floorf(x + 0.5f);
  return (int)fminf(fmaxf(r, 0.f), 255.f);
}
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(THREADS) void decode_kernel(DecArgs a) {
  __shared__ float s_q[3][64];
  __shared__ __attribute__((aligned(16))) float s_b8[8][8];       // the bases unpadded: a lane reads four or eight neighbours of a row,
  __shared__ __attribute__((aligned(16))) float s_b16[8][16];     // and the lanes of a wave share two to four addresses (broadcast)
  __shared__ __attribute__((aligned(16))) float s_f[WAVES][6][8][PF];      // dequantised coefficients [u][v]
  __shared__ float s_t[WAVES][4][8][P8];          // luma after the first product: [u][n]
  __shared__ float s_tc[WAVES][2][8][P16];        // chroma after the first product: [u][n], n < 16
  __shared__ int s_l[WAVES][4][8][P8];            // luma samples by block
  __shared__ int s_cc[WAVES][2][16][P16];         // chroma samples of the MCU

  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  if (tid < 192) s_q[tid >> 6][tid & 63] = (float)a.q[tid >> 6][tid & 63];
  if (tid < 64) s_b8[tid >> 3][tid & 7] = a.ib8[tid >> 3][tid & 7];
  if (tid < 128) s_b16[tid >> 4][tid & 15] = a.ib16[tid >> 4][tid & 15];
  __syncthreads();

  const int H = a.H, W = a.W, Hb = H >> 3, Wb = W >> 3, Hm = H >> 4, Wm = W >> 4;
  const size_t plane = (size_t)H * W;
  const int nblocks = a.nblocks;
  const int groups = (a.units + WAVES - 1) / WAVES;
  for (int g = blockIdx.x; g < groups; g += gridDim.x) {
    const int unit = g * WAVES + w;
    const bool live = unit < a.units;
    Unit u = {0, 0, 0};
    if (live && !a.gray) u = mcu_of(unit, Hm, Wm);
    // ---- 16-byte loads of the blocks, dequantised into LDS (a block the unit does not have reads as zeros)
    if (l < (a.gray ? 32 : 48)) {
      const int k = l >> 3, row = l & 7;
      const int16_t* src = nullptr;
      if (live) {
        if (a.gray) {
          const int blk = unit * 4 + k;
          if (blk < nblocks) src = a.Y + (size_t)blk * 64 + row * 8;
        } else if (k < 4) {
          src = a.Y + (((size_t)u.b * Hb + 2 * u.my + (k >> 1)) * Wb + 2 * u.mx + (k & 1)) * 64 + row * 8;
        } else {
          src = a.C + ((((size_t)u.b * 2 + (k - 4)) * Hm + u.my) * Wm + u.mx) * 64 + row * 8;
        }
      }
      int4 raw = {0, 0, 0, 0};
      if (src) raw = *reinterpret_cast<const int4*>(src);
      const int tab = k < 4 ? 0 : 1;            // one chroma table, as in libjpeg's default component setup
      const int vals[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int lo = (int)(int16_t)(vals[j] & 0xffff), hi = vals[j] >> 16;
        s_f[w][k][row][2 * j] = (float)lo * s_q[tab][row * 8 + 2 * j];
        s_f[w][k][row][2 * j + 1] = (float)hi * s_q[tab][row * 8 + 2 * j + 1];
      }
    }
    __syncthreads();
    // ---- first products: t[u][n] = sum_v F[u][v] basis[v][n]
    {
      const int k = l >> 4, uu = (l >> 1) & 7, n0 = (l & 1) * 4;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const float f = s_f[w][k][uu][v];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(f, s_b8[v][n0 + i], acc[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) s_t[w][k][uu][n0 + i] = acc[i];
    }
    if (!a.gray) {
      const int p = l >> 5, uu = (l >> 2) & 7, n0 = (l & 3) * 4;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const float f = s_f[w][4 + p][uu][v];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(f, s_b16[v][n0 + i], acc[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) s_tc[w][p][uu][n0 + i] = acc[i];
    }
    __syncthreads();
    // ---- second products: x[m][n] = sum_u basis[u][m] t[u][n], + 128, rounded and clamped per plane
    {
      const int k = l >> 4, n = l & 7, m0 = ((l >> 3) & 1) * 4;
      float acc[4] = {128.f, 128.f, 128.f, 128.f};
#pragma unroll
      for (int uu = 0; uu < 8; ++uu) {
        const float t = s_t[w][k][uu][n];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(s_b8[uu][m0 + i], t, acc[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) s_l[w][k][m0 + i][n] = sample_of(acc[i]);
    }
    if (!a.gray) {
      const int p = l >> 5, n = l & 15, m0 = ((l >> 4) & 1) * 8;
      float acc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = 128.f;
#pragma unroll
      for (int uu = 0; uu < 8; ++uu) {
        const float t = s_tc[w][p][uu][n];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(s_b16[uu][m0 + i], t, acc[i]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) s_cc[w][p][m0 + i][n] = sample_of(acc[i]);
    }
    __syncthreads();
    // ---- colour conversion and 4-byte stores
    if (a.gray) {
      const int k = l >> 4, r = (l >> 1) & 7, h4 = (l & 1) * 4;
      const int blk = unit * 4 + k;
      if (live && blk < nblocks) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) v |= (uint32_t)s_l[w][k][r][h4 + j] << (8 * j);
        const int b = blk / (Hb * Wb), rem = blk - b * Hb * Wb, by = rem / Wb, bx = rem - by * Wb;
        *reinterpret_cast<uint32_t*>(a.px + (size_t)b * plane + (size_t)(by * 8 + r) * W + bx * 8 + h4) = v;
      }
    } else if (live) {
      const int r = l >> 2, c4 = (l & 3) * 4;
      const int blk = (r >> 3) * 2 + (c4 >> 3), rr = r & 7, cc = c4 & 7;
      uint32_t R4 = 0, G4 = 0, B4 = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int yy = s_l[w][blk][rr][cc + j];
        const int cb = s_cc[w][0][r][c4 + j] - 128, cr = s_cc[w][1][r][c4 + j] - 128;
        const int R = clamp255(yy + ((__mul24(FIX16(1.402), cr) + 32768) >> 16));
        const int G = clamp255(yy + ((__mul24(-FIX16(0.344136286), cb) - __mul24(FIX16(0.714136286), cr) + 32768) >> 16));
        const int B = clamp255(yy + ((__mul24(FIX16(1.772), cb) + 32768) >> 16));
        R4 |= (uint32_t)R << (8 * j);
        G4 |= (uint32_t)G << (8 * j);
        B4 |= (uint32_t)B << (8 * j);
      }
      uint8_t* p = a.px + (size_t)u.b * 3 * plane + (size_t)(u.my * 16 + r) * W + u.mx * 16 + c4;
      *reinterpret_cast<uint32_t*>(p) = R4;
      *reinterpret_cast<uint32_t*>(p + plane) = G4;
      *reinterpret_cast<uint32_t*>(p + 2 * plane) = B4;
    }
    // s_f is rewritten next pass only after every lane has passed the last barrier, i.e. after every read of s_f and s_t
  }
}

// c(u) / div * cos((2m+1) u pi / (2 N)), in double, rounded once to fp32
static void basis(float* out, int N, double div) {
  const double pi = 3.14159265358979323846;
  for (int u = 0; u < 8; ++u)
    for (int m = 0; m < N; ++m)
      out[u * N + m] = (float)((u == 0 ? std::sqrt(0.5) : 1.0) / div * std::cos((2 * m + 1) * u * pi / (2.0 * N)));
}

// shared argument checks and the unit counts of a shape
static int check_shape(int B, int C, int H, int W, int* units, int* gray, int* nblocks) {
  if (B <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return RGBNM_EINVAL;
  const int mod = C == 3 ? 16 : 8;
  if (H % mod || W % mod) return RGBNM_EINVAL;
  if ((double)B * C * H * W >= 2147483648.0) return RGBNM_EINVAL;
  *gray = C == 1;
  *nblocks = B * (H / 8) * (W / 8);
  *units = C == 3 ? B * (H / 16) * (W / 16) : (*nblocks + 3) / 4;
  return RGBNM_OK;
}

}  // namespace pixdct

extern "C" {

int rgbnm_pixels_to_dct(const uint8_t* pixels, int B, int C, int H, int W, const int16_t* quant_host, int16_t* Y, int16_t* CbCr,
                        void* stream) {
  using namespace pixdct;
  EncArgs a;
  if (check_shape(B, C, H, W, &a.units, &a.gray, &a.nblocks) != RGBNM_OK) return RGBNM_EINVAL;
  if (!pixels || !quant_host || !Y || (C == 3 && !CbCr)) return RGBNM_EINVAL;
  if (((uintptr_t)pixels & 3) || ((uintptr_t)Y & 15) || (C == 3 && ((uintptr_t)CbCr & 15))) return RGBNM_EINVAL;
  for (int i = 0; i < C * 64; ++i)
    if (quant_host[i] < 1) return RGBNM_EINVAL;
  for (int i = 0; i < 3 * 64; ++i) a.q[i / 64][i % 64] = i < C * 64 ? quant_host[i] : (int16_t)1;
  basis(&a.fb[0][0], 16, 4.0);
  a.px = pixels; a.Y = Y; a.C = C == 3 ? CbCr : nullptr; a.H = H; a.W = W;
  const int groups = cdiv(a.units, WAVES);
  hipStream_t st = (hipStream_t)stream;
  encode_kernel<<<groups < MAX_WGS ? groups : MAX_WGS, THREADS, 0, st>>>(a);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

int rgbnm_dct_to_pixels(const int16_t* Y, const int16_t* CbCr, int B, int H, int W, const int16_t* quant_host, uint8_t* pixels,
                        void* stream) {
  using namespace pixdct;
  DecArgs a;
  const int C = CbCr ? 3 : 1;
  if (check_shape(B, C, H, W, &a.units, &a.gray, &a.nblocks) != RGBNM_OK) return RGBNM_EINVAL;
  if (!pixels || !quant_host || !Y) return RGBNM_EINVAL;
  if (((uintptr_t)pixels & 3) || ((uintptr_t)Y & 15) || ((uintptr_t)CbCr & 15)) return RGBNM_EINVAL;
  for (int i = 0; i < 3 * 64; ++i) a.q[i / 64][i % 64] = i < C * 64 ? quant_host[i] : (int16_t)1;
  basis(&a.ib8[0][0], 8, 2.0);
  basis(&a.ib16[0][0], 16, 2.0);
  a.Y = Y; a.C = CbCr; a.px = pixels; a.H = H; a.W = W;
  const int groups = cdiv(a.units, WAVES);
  hipStream_t st = (hipStream_t)stream;
  decode_kernel<<<groups < MAX_WGS ? groups : MAX_WGS, THREADS, 0, st>>>(a);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

}  // extern "C"
