// The per-run Huffman walk of the device JPEG decode (include/rgbnm.h, rgbnm_jpeg_decode_batch) as ONE __host__ __device__ body over
// plain pointers: jpeg_decode.hip runs it one lane per run, tools/jpeg_scan_check.cpp runs the very same text on the CPU under the
// host sanitizers (it defines __host__ / __device__ away).  It is libjpeg's sequential decode (jdhuff.c, decode_mcu) reshaped to one
// symbol per loop trip: the lanes of a wave are at different places of different files, and a trip that handles "the next symbol,
// whatever it is" with selects keeps them on one instruction stream; only the end of a block (store 128 bytes) is a masked branch.
//
// Safety (the bytes are untrusted):  every trip consumes at least one bit of the run or ends it with an error; the trips are bounded
// by MCUs x blocks x 64 (a trip advances the coefficient index); reads of the stream are clamped to the run's words, which
// check_run has placed inside the buffer; table look-ups are indexed by 9 bits, or range-checked; a store goes to block (by, bx) of
// a plane only if that lies inside the kept grid.  Nothing waits for another lane.
#pragma once
#include <stdint.h>

#include "../../include/rgbnm.h"

namespace jpegwalk {

// 16 bytes of the tile or of an output block; may_alias: the tile is written as int16 and moved as V16
struct __attribute__((may_alias, aligned(16))) V16 { uint32_t a, b, c, d; };

struct Out {
  int n, Hb, Wb, Hbc, Wbc;
  int16_t* Y;      // [n][Hb][Wb][64]
  int16_t* C;      // [n][2][Hbc][Wbc][64]
};

// what a lane keeps of its image record, packed for register indexing
struct Lane {
  uint64_t layout;        // 6 bits per block of the MCU: component | dx << 2 | dy << 4
  uint64_t dcsel, acsel;  // 16 bits per component: index of its table in `tabs`
  uint32_t hv;            // 8 bits per component: hs | vs << 4
  int nblk, mcus_x, ncomp;
  uint32_t total;         // MCUs of the image
};

// The run record and its image record against the buffers they index.  RGBNM_JPEG_ERECORD: the run must not be walked.
__host__ __device__ inline int check_run(const rgbnm_jpeg_run& r, const rgbnm_jpeg_image* images, int n, size_t stream_bytes,
                                         int ntables, Lane* L) {
  if (r.image < 0 || r.image >= n) return RGBNM_JPEG_ERECORD;
  const rgbnm_jpeg_image& im = images[r.image];
  if ((r.offset & 3) || r.nbytes > 0x07FFFFFFu || (uint64_t)r.offset + ((r.nbytes + 3u) & ~3u) + 4u > (uint64_t)stream_bytes)
    return RGBNM_JPEG_ERECORD;
  if ((im.ncomp != 1 && im.ncomp != 3) || im.nblk < 1 || im.nblk > 10 || im.mcus_x < 1 || im.mcus_y < 1 || im.mcus_x > 4096 ||
      im.mcus_y > 4096)
    return RGBNM_JPEG_ERECORD;
  const int64_t total = (int64_t)im.mcus_x * im.mcus_y;
  if (r.mcu0 < 0 || r.nmcu < 1 || (int64_t)r.mcu0 + r.nmcu > total || (int64_t)r.nmcu * im.nblk * 64 > 0x7FFFFFFF) return RGBNM_JPEG_ERECORD;
  uint64_t layout = 0, dcsel = 0, acsel = 0;
  uint32_t hv = 0;
  for (int c = 0; c < im.ncomp; ++c) {
    if (im.hs[c] < 1 || im.hs[c] > 4 || im.vs[c] < 1 || im.vs[c] > 4 || im.dc_tab[c] < 0 || im.dc_tab[c] >= ntables ||
        im.ac_tab[c] < 0 || im.ac_tab[c] >= ntables || ntables > 65536)
      return RGBNM_JPEG_ERECORD;
    hv |= (uint32_t)(im.hs[c] | (im.vs[c] << 4)) << (8 * c);
    dcsel |= (uint64_t)im.dc_tab[c] << (16 * c);
    acsel |= (uint64_t)im.ac_tab[c] << (16 * c);
  }
  for (int b = 0; b < im.nblk; ++b) {
    const int c = im.blk_comp[b], dx = im.blk_dx[b], dy = im.blk_dy[b];
    if (c < 0 || c >= im.ncomp || dx < 0 || dx > 3 || dy < 0 || dy > 3) return RGBNM_JPEG_ERECORD;
    layout |= (uint64_t)(c | (dx << 2) | (dy << 4)) << (6 * b);
  }
  L->layout = layout;
  L->dcsel = dcsel;
  L->acsel = acsel;
  L->hv = hv;
  L->nblk = im.nblk;
  L->mcus_x = im.mcus_x;
  L->ncomp = im.ncomp;
  L->total = (uint32_t)total;
  return 0;
}

// Store the lane's block tile (128 bytes, eight 16-byte stores) to block `blk` of MCU (my, mx) if that lies inside the kept grid,
// and leave the tile zero for the next block.
__host__ __device__ inline void flush_block(int16_t* tile, const Out& g, const Lane& L, int image, int blk, int mx, int my) {
  const int desc = (int)(L.layout >> (6 * blk)) & 63, comp = desc & 3;
  const int h = (int)(L.hv >> (8 * comp)) & 15, v = (int)(L.hv >> (8 * comp + 4)) & 15;
  const int bx = mx * h + ((desc >> 2) & 3), by = my * v + (desc >> 4);
  const int W = comp ? g.Wbc : g.Wb, H = comp ? g.Hbc : g.Hb;
  const bool ok = bx < W && by < H && (comp == 0 || g.C != nullptr);
  const size_t row = comp ? ((size_t)image * 2 + (size_t)(comp - 1)) * (size_t)H + (size_t)by : (size_t)image * (size_t)H + (size_t)by;
  V16* dst = reinterpret_cast<V16*>((comp && ok ? g.C : g.Y) + (ok ? (row * (size_t)W + (size_t)bx) * 64 : 0));
  V16* t = reinterpret_cast<V16*>(tile);
  const V16 zero = {0, 0, 0, 0};
  for (int j = 0; j < 8; ++j) {
    const V16 x = t[j];
    if (ok) dst[j] = x;
    t[j] = zero;
  }
}

// Walk one run.  tile: 64 int16 of the lane's own, 16-byte aligned, ZERO on entry and zero again on return.  tabs: the table array
// that L.dcsel / L.acsel index.  zz: zig-zag position -> natural position.  Returns 0 or a negative RGBNM_JPEG_E* code; after an
// error every block of the run that had not been stored is stored as zeros.
__host__ __device__ inline int decode_run(const uint8_t* stream, const rgbnm_jpeg_run& r, const Lane& L, const rgbnm_jpeg_hufftab* tabs,
                                          const uint8_t* zz, const Out& g, int16_t* tile) {
  const uint32_t* words = reinterpret_cast<const uint32_t*>(stream + r.offset);
  const uint32_t nwords = (r.nbytes + 3u) >> 2, total_bits = r.nbytes * 8u;
  const int image = r.image, nblk = L.nblk, mcus_x = L.mcus_x;
  uint32_t left = (uint32_t)r.nmcu;
  const uint32_t maxtrips = left * (uint32_t)nblk * 64u;
  int mx = r.mcu0 % mcus_x, my = r.mcu0 / mcus_x;
  uint64_t buf = 0;
  int have = 0, k = 0, blk = 0, err = 0;
  int p0 = 0, p1 = 0, p2 = 0;              // the DC predictors: zero at the start of every run
  uint32_t used = 0, pos = 1;
  uint32_t nextw = nwords ? words[0] : 0u;  // read one word ahead: the load's latency hides behind the trips that use the last one
  for (uint32_t trip = 0; trip < maxtrips && left; ++trip) {
    if (have <= 32) {
      buf |= (uint64_t)__builtin_bswap32(nextw) << (32 - have);
      have += 32;
      nextw = pos < nwords ? words[pos] : 0u;
      ++pos;
    }
    const int comp = (int)(L.layout >> (6 * blk)) & 3;
    const bool isdc = k == 0;
    const rgbnm_jpeg_hufftab* T = tabs + ((uint32_t)((isdc ? L.dcsel : L.acsel) >> (16 * comp)) & 0xFFFFu);
    const uint32_t e = T->look[buf >> 55];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (len == 0) {                        // a code longer than 9 bits (rare): libjpeg's canonical search
      int idx = -1;
      for (int l = 10; l <= 16; ++l) {
        const int code = (int)(buf >> (64 - l));
        if (len == 0 && code <= T->maxcode[l]) {
          len = l;
          idx = code + T->valoff[l];
        }
      }
      if (idx < 0 || idx > 255) {
        err = RGBNM_JPEG_ECODE;
        break;
      }
      sym = T->vals[idx];
    }
    const int s = sym & 15, rr = sym >> 4;
    buf <<= len;
    const uint32_t bits = (uint32_t)((buf >> 32) >> (32 - s));       // the next s bits (s = 0: none)
    buf <<= s;
    have -= len + s;
    used += (uint32_t)(len + s);
    // HUFF_EXTEND: a value below 2^(s-1) stands for value - 2^s + 1
    const int val = (s && bits < (1u << (s - 1))) ? (int)bits - (1 << s) + 1 : (int)bits;
    if (used > total_bits) {
      err = RGBNM_JPEG_EOVERRUN;
      break;
    }
    if (isdc && rr) {
      err = RGBNM_JPEG_ECODE;
      break;
    }
    p0 += (isdc && comp == 0) ? val : 0;
    p1 += (isdc && comp == 1) ? val : 0;
    p2 += (isdc && comp == 2) ? val : 0;
    const int dc = comp == 0 ? p0 : comp == 1 ? p1 : p2;
    const bool wr = isdc || s != 0;        // DC, or an AC coefficient behind a run of rr zeros; else ZRL (rr == 15) or EOB
    const int kk = isdc ? 0 : k + rr;
    if (wr) {
      if (kk > 63) {
        err = RGBNM_JPEG_EINDEX;
        break;
      }
      tile[zz[kk]] = (int16_t)(isdc ? dc : val);
    }
    k = wr ? kk + 1 : (rr == 15 ? k + 16 : 64);
    if (k >= 64) {                         // the block is complete
      flush_block(tile, g, L, image, blk, mx, my);
      k = 0;
      if (++blk == nblk) {
        blk = 0;
        --left;
        if (++mx == mcus_x) {
          mx = 0;
          ++my;
        }
      }
    }
  }
  if (!err && left) err = RGBNM_JPEG_EOVERRUN;
  if (!err && total_bits - used > 8u) err = RGBNM_JPEG_ETRAILING;
  if (err) {
    // the block under way and everything behind it: zeros (flush_block clears the tile on its first pass)
    V16* t = reinterpret_cast<V16*>(tile);
    const V16 zero = {0, 0, 0, 0};
    for (int j = 0; j < 8; ++j) t[j] = zero;
    while (left) {
      flush_block(tile, g, L, image, blk, mx, my);
      if (++blk == nblk) {
        blk = 0;
        --left;
        if (++mx == mcus_x) {
          mx = 0;
          ++my;
        }
      }
    }
  }
  return err;
}

// A one-component file has no chroma to decode: its CbCr slot is zeros.  The run over MCUs [mcu0, mcu0 + nmcu) of `total` writes
// the same share of the slot's 16-byte pieces, so that the runs of the image cover it exactly once.
__host__ __device__ inline void zero_chroma_share(const Out& g, int image, uint32_t mcu0, uint32_t nmcu, uint32_t total) {
  if (!g.C) return;
  const uint64_t pieces = (uint64_t)2 * (uint64_t)g.Hbc * (uint64_t)g.Wbc * 8u;
  const uint64_t lo = pieces * mcu0 / total, hi = pieces * ((uint64_t)mcu0 + nmcu) / total;
  V16* dst = reinterpret_cast<V16*>(g.C + (size_t)image * 2 * (size_t)g.Hbc * (size_t)g.Wbc * 64);
  const V16 zero = {0, 0, 0, 0};
  for (uint64_t j = lo; j < hi; ++j) dst[j] = zero;
}

}  // namespace jpegwalk
