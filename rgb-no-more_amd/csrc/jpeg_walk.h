// The per-run Huffman walk of the device JPEG decode (include/rgbnm.h, rgbnm_jpeg_decode_batch) as ONE __host__ __device__ body over
// plain pointers: jpeg_decode.hip runs it one lane per run, tools/jpeg_scan_check.cpp runs the very same text on the CPU under the
// host sanitizers (it defines __host__ / __device__ away).  It is libjpeg's sequential decode (jdhuff.c, decode_mcu) reshaped to one
// symbol per loop trip: the lanes of a wave are at different places of different files, and a trip that handles "the next symbol,
// whatever it is" with selects keeps them on one instruction stream; only the end of a block (store 128 bytes) is a masked branch.
// The symbol reader (Bits, next_symbol) serves the split walks of jpeg_split.h; decode_run keeps the same read written out (the comment
// above it says what the shared one cost).  A fix to one goes to the other.  Shared by every walk: the tile (zero_tile, store_tile), the
// step to the next block, the share of a one-component file's zero chroma.
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

// The lane's block tile: 128 bytes, moved as eight 16-byte pieces.
__host__ __device__ inline void zero_tile(int16_t* tile) {
  V16* t = reinterpret_cast<V16*>(tile);
  const V16 zero = {0, 0, 0, 0};
  for (int j = 0; j < 8; ++j) t[j] = zero;
}
// Move the tile to dst if `ok` and leave it zero for the next block (dst is read only if ok).
__host__ __device__ inline void store_tile(int16_t* tile, V16* dst, bool ok) {
  V16* t = reinterpret_cast<V16*>(tile);
  const V16 zero = {0, 0, 0, 0};
  for (int j = 0; j < 8; ++j) {
    const V16 x = t[j];
    if (ok) dst[j] = x;
    t[j] = zero;
  }
}

// Store the tile to block `blk` of MCU (my, mx) if that lies inside the kept grid.
__host__ __device__ inline void flush_block(int16_t* tile, const Out& g, const Lane& L, int image, int blk, int mx, int my) {
  const int desc = (int)(L.layout >> (6 * blk)) & 63, comp = desc & 3;
  const int h = (int)(L.hv >> (8 * comp)) & 15, v = (int)(L.hv >> (8 * comp + 4)) & 15;
  const int bx = mx * h + ((desc >> 2) & 3), by = my * v + (desc >> 4);
  const int W = comp ? g.Wbc : g.Wb, H = comp ? g.Hbc : g.Hb;
  const bool ok = bx < W && by < H && (comp == 0 || g.C != nullptr);
  const size_t row = comp ? ((size_t)image * 2 + (size_t)(comp - 1)) * (size_t)H + (size_t)by : (size_t)image * (size_t)H + (size_t)by;
  store_tile(tile, reinterpret_cast<V16*>((comp && ok ? g.C : g.Y) + (ok ? (row * (size_t)W + (size_t)bx) * 64 : 0)), ok);
}

// The block behind block `blk` of MCU (my, mx), in scan order.  true: it is the first of the next MCU.
__host__ __device__ inline bool next_block(const Lane& L, int& blk, int& mx, int& my) {
  if (++blk != L.nblk) return false;
  blk = 0;
  if (++mx == L.mcus_x) {
    mx = 0;
    ++my;
  }
  return true;
}

// ---- the crop form: only a box of each image is wanted (rgbnm_jpeg_decode_batch_crop) ---------------------------------------------
// The box is (top, left, h, w) in luma blocks, all even, inside the kept grid; the chroma box is the luma box halved.  The blocks of
// the box go to the image's slots of two packed buffers, luma [h][w][64] and chroma [2][h/2][w/2][64]: the layout of the host
// reader's rgbnm_read_coefficients_batch_crop.  A run starts with zero predictors at a known MCU, so a run none of whose MCUs holds
// a block of the box is not walked at all, and any other run is walked from its first MCU (predictors and bit position cannot be
// skipped) up to its LAST MCU, in raster order, that holds one.
struct Crop {
  int top, left, h, w;
  int16_t* Y;      // the image's packed luma crop [h][w][64]
  int16_t* C;      // its packed chroma crop [2][h/2][w/2][64]
};

// The box and the offsets of one image against the grids and the packed buffers.  They come from device arrays and are as little
// trusted as the run records.  RGBNM_JPEG_EBOX: nothing of the image may be stored.
__host__ __device__ inline int check_box(const int32_t* box, long long y_off, long long c_off, int Hb, int Wb, int Hbc, int Wbc,
                                         int16_t* Ypacked, size_t y_elems, int16_t* Cpacked, size_t c_elems, Crop* B) {
  const int t = box[0], l = box[1], h = box[2], w = box[3];
  if (t < 0 || l < 0 || h <= 0 || w <= 0 || ((t | l | h | w) & 1) || h > Hb || w > Wb || t > Hb - h || l > Wb - w ||
      (t + h) / 2 > Hbc || (l + w) / 2 > Wbc)
    return RGBNM_JPEG_EBOX;
  const uint64_t ny = (uint64_t)64 * (uint64_t)h * (uint64_t)w, nc = (uint64_t)128 * (uint64_t)(h / 2) * (uint64_t)(w / 2);
  if (y_off < 0 || c_off < 0 || (y_off & 7) || (c_off & 7) || (uint64_t)y_off > (uint64_t)y_elems || ny > (uint64_t)y_elems - (uint64_t)y_off ||
      (uint64_t)c_off > (uint64_t)c_elems || nc > (uint64_t)c_elems - (uint64_t)c_off)
    return RGBNM_JPEG_EBOX;
  B->top = t; B->left = l; B->h = h; B->w = w;
  B->Y = Ypacked + y_off;
  B->C = Cpacked + c_off;
  return 0;
}

// MCUs of the run to walk: up to the last one, in raster order, that holds a block of the box of some component (the box mapped
// through the component's hs / vs).  0: the run holds none and is skipped.
__host__ __device__ inline uint32_t crop_mcus(const rgbnm_jpeg_run& r, const Lane& L, const Crop& B) {
  const int end = r.mcu0 + r.nmcu - 1, mcus_x = L.mcus_x;
  int last = -1;
  for (int c = 0; c < L.ncomp; ++c) {
    const int hs = (int)(L.hv >> (8 * c)) & 15, vs = (int)(L.hv >> (8 * c + 4)) & 15;
    const int t = c ? B.top / 2 : B.top, l = c ? B.left / 2 : B.left, h = c ? B.h / 2 : B.h, w = c ? B.w / 2 : B.w;
    // the component's MCUs, inclusive (a record whose MCU grid is narrower than the call's grids is cut to its own width)
    const int x0 = l / hs, xe = (l + w - 1) / hs, x1 = xe < mcus_x ? xe : mcus_x - 1, y0 = t / vs, y1 = (t + h - 1) / vs;
    int y = end / mcus_x, x = end - y * mcus_x;
    if (y > y1) {
      y = y1;
      x = x1;
    } else if (x > x1) {
      x = x1;
    } else if (x < x0) {
      --y;
      x = x1;
    }
    const int m = y < y0 || x0 > x1 ? -1 : y * mcus_x + x;
    last = m > last ? m : last;
  }
  return last >= r.mcu0 && last <= end ? (uint32_t)(last - r.mcu0 + 1) : 0u;
}

// flush_block for the crop form: the block goes to its place in the packed crop if it lies inside its component's box.
__host__ __device__ inline void flush_block_crop(int16_t* tile, const Crop B, const Lane& L, int blk, int mx, int my) {
  const int desc = (int)(L.layout >> (6 * blk)) & 63, comp = desc & 3;
  const int h = (int)(L.hv >> (8 * comp)) & 15, v = (int)(L.hv >> (8 * comp + 4)) & 15;
  const int bt = comp ? B.top / 2 : B.top, bl = comp ? B.left / 2 : B.left, bh = comp ? B.h / 2 : B.h, bw = comp ? B.w / 2 : B.w;
  const int x = mx * h + ((desc >> 2) & 3) - bl, y = my * v + (desc >> 4) - bt;
  const bool ok = x >= 0 && x < bw && y >= 0 && y < bh;
  const size_t row = comp ? (size_t)(comp - 1) * (size_t)bh + (size_t)y : (size_t)y;
  store_tile(tile, reinterpret_cast<V16*>((comp && ok ? B.C : B.Y) + (ok ? (row * (size_t)bw + (size_t)x) * 64 : 0)), ok);
}

// ---- the symbol reader: the run's bits behind a 64-bit window, opened at any bit of the run ------------------------------------------
struct Bits {
  const uint32_t* words;
  uint32_t nwords, next;   // next: index of the word behind nextw
  uint32_t nextw;          // read one word ahead: the load's latency hides behind the trips that use the last one
  uint64_t buf;
  int have;
};

__host__ __device__ inline void bits_open(Bits& B, const uint8_t* stream, const rgbnm_jpeg_run& r, uint32_t pos) {
  B.words = reinterpret_cast<const uint32_t*>(stream + r.offset);
  B.nwords = (r.nbytes + 3u) >> 2;
  const uint32_t w = pos >> 5, off = pos & 31u;
  const uint32_t first = w < B.nwords ? B.words[w] : 0u;
  B.buf = ((uint64_t)__builtin_bswap32(first) << 32) << off;
  B.have = 32 - (int)off;
  B.nextw = w + 1 < B.nwords ? B.words[w + 1] : 0u;
  B.next = w + 2;
}

struct Sym { int len, s, rr, val; bool bad; };             // len: bits consumed in all (code and value)

// The next symbol behind table T: a 9-bit look-up, libjpeg's canonical search for the (rare) codes of 10 to 16 bits, then the s value
// bits.  bad: no code of the table matches; ONE bit is consumed then, and what the caller makes of it is the caller's.
__host__ __device__ inline Sym next_symbol(Bits& B, const rgbnm_jpeg_hufftab* T) {
  if (B.have <= 32) {
    B.buf |= (uint64_t)__builtin_bswap32(B.nextw) << (32 - B.have);
    B.have += 32;
    B.nextw = B.next < B.nwords ? B.words[B.next] : 0u;
    ++B.next;
  }
  const uint32_t e = T->look[B.buf >> 55];
  int len = (int)(e >> 8), sym = (int)(e & 255u);
  bool bad = false;
  if (len == 0) {
    int idx = -1;
    for (int l = 10; l <= 16; ++l) {
      const int code = (int)(B.buf >> (64 - l));
      if (len == 0 && code <= T->maxcode[l]) {
        len = l;
        idx = code + T->valoff[l];
      }
    }
    if (idx < 0 || idx > 255) {
      bad = true;
      len = 1;
      sym = 0;
    } else {
      sym = T->vals[idx];
    }
  }
  Sym o;
  o.s = sym & 15;
  o.rr = sym >> 4;
  B.buf <<= len;
  const uint32_t bits = (uint32_t)((B.buf >> 32) >> (32 - o.s));   // the next s bits (s = 0: none)
  B.buf <<= o.s;
  B.have -= len + o.s;
  o.len = len + o.s;
  // HUFF_EXTEND: a value below 2^(s-1) stands for value - 2^s + 1
  o.val = (o.s && bits < (1u << (o.s - 1))) ? (int)bits - (1 << o.s) + 1 : (int)bits;
  o.bad = bad;
  return o;
}

__host__ __device__ inline const rgbnm_jpeg_hufftab* table_of(const Lane& L, const rgbnm_jpeg_hufftab* tabs, int comp, bool isdc) {
  return tabs + ((uint32_t)((isdc ? L.dcsel : L.acsel) >> (16 * comp)) & 0xFFFFu);
}

// Walk one run.  tile: 64 int16 of the lane's own, 16-byte aligned, ZERO on entry and zero again on return.  tabs: the table array
// that L.dcsel / L.acsel index.  zz: zig-zag position -> natural position.  Returns 0 or a negative RGBNM_JPEG_E* code; after an
// error every block of the run that had not been stored is stored as zeros.
// CROP (a compile-time choice: the plain walk carries no trace of it): only the first nwalk MCUs (crop_mcus) are walked and the
// blocks go through flush_block_crop.  A walk that stops before the run's end has not seen the run's tail, so the two checks behind
// the loop are not made for it; the errors it does meet are the ones the plain walk meets first, with the same codes.
// The symbol read is written out here and not taken from next_symbol below: on top of next_symbol the one-lane launches measured up to
// 2.6 % (plain, no restart markers) and 6 - 8 % (crop) slower than with this text, against a run-to-run disagreement below 1 %.
// The template is the function itself, with defaults, and not a body behind a decode_run wrapper: with the wrapper the plain kernel's
// assembly differed in four instruction encodings and the launch time moved by 1 - 8 %; this way it is what it was without the crop form.
template <bool CROP = false>
__host__ __device__ inline int decode_run(const uint8_t* stream, const rgbnm_jpeg_run& r, const Lane& L, const rgbnm_jpeg_hufftab* tabs,
                                          const uint8_t* zz, const Out& g, int16_t* tile, const Crop B = Crop(), uint32_t nwalk = 0u) {
  const uint32_t* words = reinterpret_cast<const uint32_t*>(stream + r.offset);
  const uint32_t nwords = (r.nbytes + 3u) >> 2, total_bits = r.nbytes * 8u;
  const int image = r.image, nblk = L.nblk, mcus_x = L.mcus_x;
  uint32_t left = CROP ? nwalk : (uint32_t)r.nmcu;
  const bool early = CROP && nwalk < (uint32_t)r.nmcu;
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
      if (CROP) flush_block_crop(tile, B, L, blk, mx, my);
      else flush_block(tile, g, L, image, blk, mx, my);
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
  if (!early && !err && left) err = RGBNM_JPEG_EOVERRUN;
  if (!early && !err && total_bits - used > 8u) err = RGBNM_JPEG_ETRAILING;
  if (err || (CROP && left)) {
    // the block under way and everything behind it: zeros (flush_block clears the tile on its first pass)
    V16* t = reinterpret_cast<V16*>(tile);
    const V16 zero = {0, 0, 0, 0};
    for (int j = 0; j < 8; ++j) t[j] = zero;
    while (left) {
      if (CROP) flush_block_crop(tile, B, L, blk, mx, my);
      else flush_block(tile, g, L, image, blk, mx, my);
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

// The crop form.  nwalk: crop_mcus(r, L, B), not 0.  After an error only the blocks still owed -- those of the nwalk MCUs -- are zeroed.
__host__ __device__ inline int decode_run_crop(const uint8_t* stream, const rgbnm_jpeg_run& r, const Lane& L, const rgbnm_jpeg_hufftab* tabs,
                                               const uint8_t* zz, const Crop& B, uint32_t nwalk, int16_t* tile) {
  const Out none = {0, 0, 0, 0, 0, nullptr, nullptr};
  return decode_run<true>(stream, r, L, tabs, zz, none, tile, B, nwalk);
}

// A one-component file has no chroma to decode: its CbCr slot is zeros, written as 16-byte pieces.  The run over MCUs
// [mcu0, mcu0 + nmcu) of `total` takes the same share [lo, hi) of the slot's `pieces`, so that the runs of the image cover it exactly once.
struct Pieces { uint64_t lo, hi; };
__host__ __device__ inline Pieces chroma_share(uint64_t pieces, uint32_t mcu0, uint32_t nmcu, uint32_t total) {
  const Pieces p = {pieces * mcu0 / total, pieces * ((uint64_t)mcu0 + nmcu) / total};
  return p;
}
__host__ __device__ inline void zero_pieces(int16_t* slot, Pieces p) {
  V16* dst = reinterpret_cast<V16*>(slot);
  const V16 zero = {0, 0, 0, 0};
  for (uint64_t j = p.lo; j < p.hi; ++j) dst[j] = zero;
}
__host__ __device__ inline uint64_t chroma_pieces(const Out& g) { return (uint64_t)2 * (uint64_t)g.Hbc * (uint64_t)g.Wbc * 8u; }
__host__ __device__ inline int16_t* chroma_slot(const Out& g, int image) { return g.C + (size_t)image * 2 * (size_t)g.Hbc * (size_t)g.Wbc * 64; }

__host__ __device__ inline void zero_chroma_share(const Out& g, int image, uint32_t mcu0, uint32_t nmcu, uint32_t total) {
  if (g.C) zero_pieces(chroma_slot(g, image), chroma_share(chroma_pieces(g), mcu0, nmcu, total));
}
// The packed chroma crop: every run of the image takes its share, whether it is walked or skipped.
__host__ __device__ inline void zero_chroma_share_crop(const Crop& B, uint32_t mcu0, uint32_t nmcu, uint32_t total) {
  zero_pieces(B.C, chroma_share((uint64_t)2 * (uint64_t)(B.h / 2) * (uint64_t)(B.w / 2) * 8u, mcu0, nmcu, total));
}

}  // namespace jpegwalk
