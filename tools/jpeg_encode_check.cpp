// Stand-alone host check of the shared JPEG emit code (rgb-no-more_amd/csrc/jpeg_emit.h): encodes coefficient dumps to JPEG files
// with the very functions the kernels of csrc/jpeg_encode.hip call, in the kernels' four steps, so that the sanitizers see them.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_encode_check.cpp -o jpeg_encode_check
//   jpeg_encode_check IN OUT [IN OUT ...]
//
// IN: int32 ncomp, height, width, restart; int16 quant [ncomp][64]; int16 Y [Hb][Wb][64]; for three components int16 CbCr
// [2][Hbc][Wbc][64] -- the grids are the kept grids of height x width at 4:2:0.  OUT: the file.  Prints one line per input:
// "<IN> ok <bytes>" or "<IN> status <code>" (then no file is written).  tests/test_jpeg_encode_cpu.py compares the files.
//
// Unlike the device, this program places and emits the blocks in an order of its own choosing: the positions come from the same
// function composition, cut into trips of 5 blocks, and the blocks are emitted LAST FIRST, which the OR merge must not notice.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define __host__
#define __device__
#include "../rgb-no-more_amd/csrc/jpeg_emit.h"

using namespace jpegemit;

static constexpr Std STD = JPEGEMIT_STD_INIT;
static constexpr Codes CODES = make_codes(STD);

struct Image {
  Geo g;
  int height, width;
  std::vector<int16_t> quant, Y, C;
};

struct WordMem {
  std::vector<uint32_t> words;
  void set_word(uint32_t i, uint32_t v) { if (i < words.size()) words[i] = v; }
  void or_word(uint32_t i, uint32_t v) { if (i < words.size()) words[i] |= v; }
};
struct OutBytes {
  std::vector<uint8_t>& v;
  void put(uint32_t pos, uint8_t b) { if (pos < v.size()) v[pos] = b; }
};

static bool read_image(const char* path, Image& im) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[4];
  bool ok = fread(h, 4, 4, f) == 4;
  if (ok) {
    im.height = h[1]; im.width = h[2];
    ok = h[1] >= 1 && h[2] >= 1 && h[1] <= 65535 && h[2] <= 65535 &&
         make_geo(im.g, cdiv(h[1], 8), cdiv(h[2], 8), cdiv(h[1], 16), cdiv(h[2], 16), h[0], h[3]);
  }
  if (ok) {
    im.quant.resize((size_t)im.g.ncomp * 64);
    im.Y.resize((size_t)im.g.Hb * im.g.Wb * 64);
    im.C.resize(im.g.ncomp == 3 ? (size_t)2 * im.g.Hbc * im.g.Wbc * 64 : 0);
    ok = fread(im.quant.data(), 2, im.quant.size(), f) == im.quant.size() && fread(im.Y.data(), 2, im.Y.size(), f) == im.Y.size() &&
         fread(im.C.data(), 2, im.C.size(), f) == im.C.size();
  }
  fclose(f);
  return ok;
}

// 0 and the file in `out`, or the status the device would give
static int encode(const Image& im, std::vector<uint8_t>& out) {
  const Geo& g = im.g;
  if (!dims_fit(g, im.height, im.width)) return ST_EGRID;
  for (size_t i = 0; i < (g.ncomp == 3 ? 128u : 64u); ++i)
    if (im.quant[i] < 1 || im.quant[i] > 255) return ST_ERANGE;
  auto dc = [&](int comp, int by, int bx) { return (int)(comp ? im.C : im.Y)[coef_offset(g, 0, comp, by, bx)]; };
  auto coded = [&](int b, auto& sink) {
    const Blk k = block_at(g, b);
    const int16_t* p = k.real ? (k.comp ? im.C : im.Y).data() + coef_offset(g, 0, k.comp, k.by, k.bx) : nullptr;
    return code_block(CODES, k.comp ? 1 : 0, dc_diff(g, k, dc), k.real, [p](int i) { return (int)p[i]; }, sink);
  };
  // 1 measure
  std::vector<uint32_t> pos(g.nblocks);
  bool bad = false;
  for (int b = 0; b < g.nblocks; ++b) {
    BitCount cnt;
    if (coded(b, cnt)) pos[b] = cnt.bits; else { pos[b] = 0; bad = true; }
  }
  if (bad) return ST_ERANGE;
  // 2 place, in trips of 5 blocks
  const int per_run = g.ri * g.nblk, TRIP = 5;
  std::vector<uint32_t> run_start(g.nruns + 1);
  uint32_t carry = 0;
  for (int base = 0; base < g.nblocks; base += TRIP) {
    Fn f{0, 0, 0};
    for (int b = base; b < base + TRIP && b < g.nblocks; ++b) {
      const uint32_t len = pos[b];
      const bool first = b % per_run == 0;
      f = compose(f, Fn{0, len, first ? 1u : 0u});
      pos[b] = apply(f, carry) - len;
      if (first) run_start[b / per_run] = pos[b] >> 3;
    }
    carry = apply(f, carry);
  }
  const uint32_t rawbytes = align8(carry) >> 3;
  run_start[g.nruns] = rawbytes;
  // 3 emit, last block first
  WordMem mem;
  mem.words.assign((rawbytes + 3) / 4 + 4, 0);
  for (int b = g.nblocks - 1; b >= 0; --b) {
    BitSink<WordMem> sink(mem, pos[b]);
    coded(b, sink);
    if ((b + 1) % per_run == 0 || b + 1 == g.nblocks) sink.pad_to_byte();
    sink.flush();
  }
  std::vector<uint8_t> raw(mem.words.size() * 4);
  for (size_t i = 0; i < mem.words.size(); ++i)
    for (int k = 0; k < 4; ++k) raw[4 * i + k] = (uint8_t)(mem.words[i] >> (24 - 8 * k));
  // 4 stuff and assemble, 16 raw bytes at a time
  uint32_t nff = 0;
  for (size_t i = 0; i < mem.words.size(); ++i) nff += count_ff(mem.words[i]);
  const uint32_t hdr = (uint32_t)header_bytes(g);
  out.assign(file_size(g, rawbytes, nff), 0xAA);
  OutBytes ob{out};
  for (uint32_t i = 0; i < hdr; ++i) ob.put(i, header_byte(STD, g, (int)i, im.height, im.width, im.quant.data()));
  uint32_t before = 0;
  for (uint32_t i0 = 0; i0 < rawbytes; i0 += 16) {
    const uint32_t i1 = i0 + 16 < rawbytes ? i0 + 16 : rawbytes;
    stuff_chunk(raw.data(), i0, i1, run_start.data(), g.nruns, before, hdr, ob);
    for (uint32_t i = i0; i < i1; ++i) before += raw[i] == 0xFF;
  }
  if (before != nff) return -1;
  out[out.size() - 2] = 0xFF;
  out[out.size() - 1] = 0xD9;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3 || (argc - 1) % 2) {
    fprintf(stderr, "usage: %s IN OUT [IN OUT ...]\n", argv[0]);
    return 2;
  }
  for (int k = 1; k + 1 < argc; k += 2) {
    Image im;
    if (!read_image(argv[k], im)) {
      fprintf(stderr, "%s: cannot read\n", argv[k]);
      return 2;
    }
    std::vector<uint8_t> out;
    const int st = encode(im, out);
    if (st != 0) {
      printf("%s status %d\n", argv[k], st);
      continue;
    }
    FILE* f = fopen(argv[k + 1], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) {
      fprintf(stderr, "%s: cannot write\n", argv[k + 1]);
      return 2;
    }
    fclose(f);
    printf("%s ok %zu\n", argv[k], out.size());
  }
  return 0;
}
