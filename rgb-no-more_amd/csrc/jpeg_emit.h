// Baseline JPEG entropy ENCODING, the parts that are plain C++ (include/rgbnm.h: rgbnm_jpeg_encode_batch): shared by the kernels
// of jpeg_encode.hip and by the stand-alone host check tools/jpeg_encode_check.cpp, which runs the same code under the sanitizers.
//
// The file written is the one libjpeg's transcoder (jpeg_write_coefficients) writes with its defaults: JFIF APP0, one DQT segment per
// table, SOF0, 4:2:0 or one component, one DHT segment per T.81 Annex K table, optionally DRI, one interleaved scan.
//
//   Geo / block_at      the scan order: block b of an image -> component and position on the MCU-PADDED grid
//   dc_diff             a block's DC difference, its predecessor found by index (no walk); the padding rule of libjpeg's transcoder:
//                       a block beyond the kept grid has zero AC and the DC of the block before it in the MCU, so its difference is 0
//   code_block          zig-zag, run/size symbols, ZRL, EOB, size and extra bits, code lookup -- into a sink (BitCount or BitSink)
//   Fn / compose        the bit position of every block as a prefix "sum" of functions: x + s, or at the first block of a restart run
//                       align8(x) + s; such functions compose associatively, so one scan places all blocks of an image
//   BitSink             writes a block's bits at its position: whole 32-bit words are stored, the first and last word, which a
//                       neighbour shares, are merged by integer OR into zeroed memory (order-independent: the bytes never vary)
//   count_ff / stuff_chunk   FF -> FF 00, RSTn between the runs
//   header_byte         byte i of the header, SOI through the SOS header
#pragma once
#include <stddef.h>
#include <stdint.h>

// a host program that includes this header defines __host__ / __device__ away first (tools/jpeg_encode_check.cpp)
#define JE_HD __host__ __device__ inline

namespace jpegemit {

constexpr int BLOCK_BITS_MAX = 1660;       // 22 (longest DC code 11 + 11 extra bits, chroma) + 63 * 26 (longest AC code 16 + 10)
constexpr int HDR3 = 623, HDR1 = 328;      // header bytes of a three- / one-component file without DRI
constexpr int DRI_BYTES = 6;
constexpr int GRID_MAX = 4096;
constexpr uint32_t LEN_ERANGE = 0xffffffffu;   // a block's length when a value does not fit baseline Huffman coding

// per-image status codes (include/rgbnm.h)
constexpr int ST_EGRID = -13, ST_ECAPACITY = -15, ST_ERANGE = -25;

JE_HD constexpr int zz(int k) {            // natural index of zig-zag position k
  constexpr uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k];
}

// T.81 Annex K.3: table 0 luminance, table 1 chrominance
struct Std {
  uint8_t dc_bits[2][16], dc_vals[2][12], ac_bits[2][16], ac_vals[2][162];
};
#define JPEGEMIT_STD_INIT                                                                                                           \
  {                                                                                                                                 \
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}},                           \
        {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},                                           \
        {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}},                 \
    {                                                                                                                               \
      {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, \
       0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, \
       0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, \
       0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, \
       0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, \
       0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, \
       0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, \
       0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},                                   \
      {                                                                                                                             \
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,     \
            0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, \
            0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, \
            0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, \
            0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, \
            0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, \
            0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, \
            0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, \
            0xf9, 0xfa                                                                                                              \
      }                                                                                                                             \
    }                                                                                                                               \
  }

// (code << 8) | length of every symbol; 0: the table has no code for it (T.81 Annex C)
struct Codes {
  uint32_t dc[2][12], ac[2][256];
};
constexpr Codes make_codes(const Std& s) {
  Codes c{};
  for (int t = 0; t < 2; ++t) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < s.dc_bits[t][len - 1]; ++i) c.dc[t][s.dc_vals[t][k++]] = (code++ << 8) | (uint32_t)len;
      code <<= 1;
    }
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < s.ac_bits[t][len - 1]; ++i) c.ac[t][s.ac_vals[t][k++]] = (code++ << 8) | (uint32_t)len;
      code <<= 1;
    }
  }
  return c;
}

// ---- geometry ---------------------------------------------------------------------------------------------------------------------
JE_HD int cdiv(int a, int b) { return (a + b - 1) / b; }

// One batch: every image has the same kept grids, so the same MCU grid.  4:2:0: an MCU is Y (0,0) (0,1) (1,0) (1,1), Cb, Cr; the
// chroma grids equal the MCU grid and only luma can have padding (an odd Hb or Wb).  One component: an MCU is a block, no padding.
struct Geo {
  int ncomp, Hb, Wb, Hbc, Wbc, mcus_x, mcus_y, nblk, nmcu;
  int restart;                             // as given: the DRI value (0: none)
  int ri, nruns;                           // MCUs per run (nmcu without restarts), runs per image
  int nblocks;                             // nmcu * nblk
};
// false: not a grid this encoder takes.  The limit on the block count keeps every bit position of an image inside 32 bits.
JE_HD bool make_geo(Geo& g, int Hb, int Wb, int Hbc, int Wbc, int ncomp, int restart) {
  if ((ncomp != 1 && ncomp != 3) || Hb < 1 || Wb < 1 || Hb > GRID_MAX || Wb > GRID_MAX || restart < 0 || restart > 65535) return false;
  if (ncomp == 3 && (Hbc != (Hb + 1) / 2 || Wbc != (Wb + 1) / 2)) return false;
  g.ncomp = ncomp; g.Hb = Hb; g.Wb = Wb; g.Hbc = ncomp == 3 ? Hbc : 0; g.Wbc = ncomp == 3 ? Wbc : 0;
  g.mcus_x = ncomp == 3 ? Wbc : Wb;
  g.mcus_y = ncomp == 3 ? Hbc : Hb;
  g.nblk = ncomp == 3 ? 6 : 1;
  g.nmcu = g.mcus_x * g.mcus_y;
  g.restart = restart;
  g.ri = restart == 0 || restart > g.nmcu ? g.nmcu : restart;
  g.nruns = cdiv(g.nmcu, g.ri);
  const unsigned long long bits = (unsigned long long)g.nmcu * g.nblk * BLOCK_BITS_MAX + 8ull * g.nruns + 64;
  if (bits >= (1ull << 32)) return false;
  g.nblocks = g.nmcu * g.nblk;
  return true;
}
JE_HD int header_bytes(const Geo& g) { return (g.ncomp == 3 ? HDR3 : HDR1) + (g.restart ? DRI_BYTES : 0); }
// The kept grids of a height x width image at this sampling
JE_HD bool dims_fit(const Geo& g, int height, int width) {
  if (height < 1 || width < 1 || height > 65535 || width > 65535) return false;
  if (cdiv(height, 8) != g.Hb || cdiv(width, 8) != g.Wb) return false;
  return g.ncomp == 1 || (cdiv(height, 16) == g.Hbc && cdiv(width, 16) == g.Wbc);
}
// Worst-case file size: every block at its longest, every scan byte FF
JE_HD size_t file_bound(const Geo& g) {
  return (size_t)header_bytes(g) + 2 * ((size_t)g.nblocks * ((BLOCK_BITS_MAX + 7) / 8)) + 2 * (size_t)(g.nruns - 1) + 2;
}

struct Blk {
  int mcu, j, comp, by, bx;                // block j of the MCU; position on the component's padded grid
  bool real;                               // inside the kept grid
};
JE_HD Blk block_at(const Geo& g, int b) {
  Blk k;
  k.mcu = b / g.nblk;
  k.j = b - k.mcu * g.nblk;
  const int my = k.mcu / g.mcus_x, mx = k.mcu - my * g.mcus_x;
  if (g.ncomp == 3 && k.j < 4) {
    k.comp = 0; k.by = 2 * my + (k.j >> 1); k.bx = 2 * mx + (k.j & 1);
    k.real = k.by < g.Hb && k.bx < g.Wb;
  } else {
    k.comp = g.ncomp == 3 ? k.j - 3 : 0; k.by = my; k.bx = mx;
    k.real = true;
  }
  return k;
}
// Element offset of a real block's 64 coefficients: comp 0 in Y [n][Hb][Wb][64], comp 1 / 2 in CbCr [n][2][Hbc][Wbc][64]
JE_HD size_t coef_offset(const Geo& g, int img, int comp, int by, int bx) {
  if (comp == 0) return (((size_t)img * g.Hb + by) * g.Wb + bx) * 64;
  return ((((size_t)img * 2 + (comp - 1)) * g.Hbc + by) * g.Wbc + bx) * 64;
}

// DC of luma block j of an MCU as the transcoder codes it: its own when it is real, else that of the block before it in the MCU.
// Block 0 of an MCU is always real.  dc(comp, by, bx) reads a real block's DC.
template <class DC>
JE_HD int luma_dc(const Geo& g, int mcu, int j, DC dc) {
  const int my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
  for (; j > 0; --j) {
    const int by = 2 * my + (j >> 1), bx = 2 * mx + (j & 1);
    if (by < g.Hb && bx < g.Wb) return dc(0, by, bx);
  }
  return dc(0, 2 * my, 2 * mx);
}
// The DC difference of a block: against the block of the same component before it in scan order, 0 at the start of a restart run.
template <class DC>
JE_HD int dc_diff(const Geo& g, const Blk& k, DC dc) {
  if (!k.real) return 0;                   // padding: the DC of the block before it, coded against that block
  const bool first = k.mcu % g.ri == 0;
  const int own = dc(k.comp, k.by, k.bx);
  int pred;
  if (g.ncomp == 3 && k.comp == 0)
    pred = k.j > 0 ? luma_dc(g, k.mcu, k.j - 1, dc) : first ? 0 : luma_dc(g, k.mcu - 1, 3, dc);
  else
    pred = first ? 0 : dc(k.comp, (k.mcu - 1) / g.mcus_x, (k.mcu - 1) % g.mcus_x);
  return own - pred;
}

// ---- one block's symbols ----------------------------------------------------------------------------------------------------------
JE_HD int bit_size(int v) {                // T.81 F.1.2.1: the category of a value
  const unsigned a = v < 0 ? (unsigned)-v : (unsigned)v;
  return a ? 32 - __builtin_clz(a) : 0;
}
JE_HD uint32_t extra_bits(int v, int s) { return (uint32_t)(v >= 0 ? v : v + (1 << s) - 1); }

struct BitCount {
  uint32_t bits = 0;
  JE_HD void put(uint32_t, int len) { bits += (uint32_t)len; }
};

// Codes one block into `sink`: ac(i) is the coefficient at NATURAL index i (not called for padding).  tab: 0 luma, 1 chroma.
// false: the DC difference needs more than 11 bits or an AC coefficient more than 10 (the sink then holds a partial block).
template <class AC, class Sink>
JE_HD bool code_block(const Codes& t, int tab, int diff, bool real, const AC& ac, Sink& sink) {
  int s = bit_size(diff);
  if (s > 11) return false;
  uint32_t c = t.dc[tab][s];
  sink.put(c >> 8, (int)(c & 255));
  if (s) sink.put(extra_bits(diff, s), s);
  int zeros = 0;
  bool ok = true;
  if (real) {
#pragma unroll
    for (int k = 1; k < 64; ++k) {
      const int v = ac(zz(k));
      if (v == 0) { ++zeros; continue; }
      while (zeros > 15) {
        c = t.ac[tab][0xF0];
        sink.put(c >> 8, (int)(c & 255));
        zeros -= 16;
      }
      s = bit_size(v);
      if (s > 10) { ok = false; s = 10; }
      c = t.ac[tab][(zeros << 4) | s];
      sink.put(c >> 8, (int)(c & 255));
      sink.put(extra_bits(v, s) & ((1u << s) - 1), s);
      zeros = 0;
    }
  } else {
    zeros = 63;
  }
  if (zeros) {
    c = t.ac[tab][0];
    sink.put(c >> 8, (int)(c & 255));
  }
  return ok;
}

// ---- placing the blocks -----------------------------------------------------------------------------------------------------------
JE_HD uint32_t align8(uint32_t x) { return (x + 7u) & ~7u; }
// x -> f ? align8(x + a) + s : x + s.  A block of `len` bits is {0, len, first block of a run}; applying the composition of blocks
// 0..b to 0 gives the bit position behind block b in the image's raw stream, whose runs each start on a byte.
struct Fn {
  uint32_t a, s, f;
};
JE_HD uint32_t apply(const Fn& p, uint32_t x) { return p.f ? align8(x + p.a) + p.s : x + p.s; }
JE_HD Fn compose(const Fn& p, const Fn& q) {        // p first, then q
  if (!q.f) return Fn{p.a, p.s + q.s, p.f};
  if (!p.f) return Fn{p.s + q.a, q.s, 1u};
  return Fn{p.a, align8(p.s + q.a) + q.s, 1u};      // align8(align8(x + a) + y) = align8(x + a) + align8(y)
}

// ---- writing a block's bits -------------------------------------------------------------------------------------------------------
// Mem: set_word(index, value) / or_word(index, value) on 32-bit words holding four stream bytes, first byte in the top bits; both
// check the index against the buffer.
template <class Mem>
struct BitSink {
  Mem& m;
  uint64_t acc;
  uint32_t w;                              // word being filled
  int n;                                   // bits of it filled
  bool shared;                             // a neighbour writes this word too
  JE_HD BitSink(Mem& mem, uint32_t bitpos) : m(mem), acc(0), w(bitpos >> 5), n((int)(bitpos & 31)), shared((bitpos & 31) != 0) {}
  JE_HD void put(uint32_t v, int len) {
    acc = (acc << len) | v;
    n += len;
    if (n >= 32) {
      n -= 32;
      const uint32_t x = (uint32_t)(acc >> n);
      if (shared) m.or_word(w, x); else m.set_word(w, x);
      shared = false;
      ++w;
    }
  }
  JE_HD uint32_t position() const { return w * 32u + (uint32_t)n; }
  JE_HD void pad_to_byte() {               // T.81 F.1.2.3: 1-bits
    const int pad = (int)(-(int)position() & 7);
    if (pad) put((1u << pad) - 1, pad);
  }
  JE_HD void flush() {
    if (n > 0) m.or_word(w, (uint32_t)(acc << (32 - n)));
  }
};

// ---- stuffing and assembly --------------------------------------------------------------------------------------------------------
JE_HD uint32_t count_ff(uint32_t word) {
  return (uint32_t)((word & 0xffu) == 0xffu) + (uint32_t)((word & 0xff00u) == 0xff00u) + (uint32_t)((word & 0xff0000u) == 0xff0000u) +
         (uint32_t)((word & 0xff000000u) == 0xff000000u);
}
JE_HD uint32_t file_size(const Geo& g, uint32_t rawbytes, uint32_t nff) { return (uint32_t)header_bytes(g) + rawbytes + nff + 2u * (uint32_t)g.nruns; }

// Raw bytes [i0, i1) of an image to their places in the file.  run_start[r]: the raw byte at which run r begins (increasing; every
// run has at least one byte); ff_before: FF bytes in raw[0, i0).  Byte i of run r lands at header + i + (FFs before it) + 2 r, the
// marker FF D0+((r-1)&7) in the two bytes before run r's first.  out.put(position, byte) checks the position.
template <class Out>
JE_HD void stuff_chunk(const uint8_t* raw, uint32_t i0, uint32_t i1, const uint32_t* run_start, int nruns, uint32_t ff_before,
                       uint32_t header, Out& out) {
  if (i0 >= i1) return;
  int lo = 0, hi = nruns - 1;
  while (lo < hi) {                        // the last run that starts at or before i0
    const int mid = (lo + hi + 1) >> 1;
    if (run_start[mid] <= i0) lo = mid; else hi = mid - 1;
  }
  int r = lo;
  uint32_t begin = run_start[r];
  uint32_t next = r + 1 < nruns ? run_start[r + 1] : 0xffffffffu;
  uint32_t pos = header + i0 + ff_before + 2u * (uint32_t)r;
  for (uint32_t i = i0; i < i1; ++i) {
    if (i == next) {
      ++r;
      begin = next;
      next = r + 1 < nruns ? run_start[r + 1] : 0xffffffffu;
      pos += 2;
    }
    if (i == begin && r > 0) {
      out.put(pos - 2, 0xFF);
      out.put(pos - 1, (uint8_t)(0xD0 + ((r - 1) & 7)));
    }
    const uint8_t v = raw[i];
    out.put(pos++, v);
    if (v == 0xFF) out.put(pos++, 0);
  }
}

// ---- header -----------------------------------------------------------------------------------------------------------------------
// Byte i (0 <= i < header_bytes) of the file of a height x width image; quant: int16 [ncomp][64] in natural order (table 1 serves
// both chroma components; values are written as 8 bits).
JE_HD uint8_t header_byte(const Std& std_, const Geo& g, int i, int height, int width, const int16_t* quant) {
  constexpr uint8_t head[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 0x4A, 0x46, 0x49, 0x46, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00};
  if (i < 20) return head[i];
  i -= 20;
  const int ntab = g.ncomp == 3 ? 2 : 1;
  for (int t = 0; t < ntab; ++t) {         // DQT
    if (i < 69) {
      if (i < 5) { const uint8_t h[5] = {0xFF, 0xDB, 0x00, 0x43, (uint8_t)t}; return h[i]; }
      return (uint8_t)quant[t * 64 + zz(i - 5)];
    }
    i -= 69;
  }
  const int sof = 10 + 3 * g.ncomp;        // SOF0
  if (i < sof) {
    if (i < 10) {
      const uint8_t h[10] = {0xFF, 0xC0, 0x00, (uint8_t)(8 + 3 * g.ncomp), 8, (uint8_t)(height >> 8), (uint8_t)height, (uint8_t)(width >> 8),
                             (uint8_t)width, (uint8_t)g.ncomp};
      return h[i];
    }
    const int c = (i - 10) / 3, f = (i - 10) % 3;
    return f == 0 ? (uint8_t)(c + 1) : f == 1 ? (uint8_t)(g.ncomp == 3 && c == 0 ? 0x22 : 0x11) : (uint8_t)(c ? 1 : 0);
  }
  i -= sof;
  for (int t = 0; t < ntab; ++t) {         // DHT: DC t, AC t
    if (i < 33) {
      if (i < 5) { const uint8_t h[5] = {0xFF, 0xC4, 0x00, 0x1F, (uint8_t)t}; return h[i]; }
      return i < 21 ? std_.dc_bits[t][i - 5] : std_.dc_vals[t][i - 21];
    }
    i -= 33;
    if (i < 183) {
      if (i < 5) { const uint8_t h[5] = {0xFF, 0xC4, 0x00, 0xB5, (uint8_t)(0x10 | t)}; return h[i]; }
      return i < 21 ? std_.ac_bits[t][i - 5] : std_.ac_vals[t][i - 21];
    }
    i -= 183;
  }
  if (g.restart) {                         // DRI
    if (i < 6) { const uint8_t h[6] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(g.restart >> 8), (uint8_t)g.restart}; return h[i]; }
    i -= 6;
  }
  if (i < 5) { const uint8_t h[5] = {0xFF, 0xDA, 0x00, (uint8_t)(6 + 2 * g.ncomp), (uint8_t)g.ncomp}; return h[i]; }   // SOS
  i -= 5;
  if (i < 2 * g.ncomp) return (i & 1) == 0 ? (uint8_t)(i / 2 + 1) : (uint8_t)(i / 2 ? 0x11 : 0x00);
  i -= 2 * g.ncomp;
  return i == 1 ? 63 : 0;
}

}  // namespace jpegemit
