// What the stand-alone host checks of the device JPEG decode share (jpeg_scan_check.cpp, jpeg_split_check.cpp, jpeg_crop_check.cpp;
// each stays a program of its own, built with the host sanitizers as its first lines say): the device headers compiled for the CPU,
// an input file with its grid, one file's plan through jpegscan::prepare in heap blocks of the exact size, the one-lane reference walk,
// and the input driver -- every file as given, every truncation length of the first two, 6000 single-byte mutations from a fixed seed
// (--share D: every D-th truncation and mutation only).  The comparisons and the tallies are the programs' own.
#pragma once
#define __host__
#define __device__
#include "../rgb-no-more_amd/csrc/jpeg_scan.h"
#include "../rgb-no-more_amd/csrc/jpeg_walk.h"

#include <cstdio>
#include <cstdlib>
#include <string>

namespace jpegcheck {

static const int16_t SENTINEL = 0x5555;                        // what an output holds before the walk: no element may keep it

struct File {
  std::string name;
  std::vector<uint8_t> bytes;
  int Hb = 0, Wb = 0;
  bool refused() const { return name.size() >= 12 && name.compare(name.size() - 12, 12, "_refused.jpg") == 0; }
};

[[noreturn]] static void fail(const char* what) {
  fprintf(stderr, "%s\n", what);
  exit(1);
}

// grid of the frame header, for the call's Hb / Wb (component 0 has the largest sampling factors in the files this is fed)
static bool grid_of(const std::vector<uint8_t>& d, int* Hb, int* Wb) {
  for (size_t p = 2; p + 9 < d.size();) {
    if (d[p] != 0xFF) return false;
    const int m = d[p + 1], len = (d[p + 2] << 8) | d[p + 3];
    if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
      *Hb = (((d[p + 5] << 8) | d[p + 6]) + 7) / 8;
      *Wb = (((d[p + 7] << 8) | d[p + 8]) + 7) / 8;
      return true;
    }
    p += 2 + (size_t)len;
  }
  return false;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;             // xorshift64, fixed seed
static uint64_t next() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// One file's plan.  Not copied: p points into the vectors.
struct Plan {
  std::vector<uint8_t> stream;
  std::vector<rgbnm_jpeg_run> runs;
  std::vector<rgbnm_jpeg_hufftab> tables;
  rgbnm_jpeg_image image;
  rgbnm_jpeg_plan p;
  int Hb, Wb, Hbc, Wbc;
};

// Fill P from the file's bytes (an exact-size copy of them).  Returns the parser's status: 0, or its refusal, which carries a message.
// An accepted plan keeps the used prefix of the stream alone, as the device holds it: the sanitizer sees any read past it.
static int prepare(Plan& P, const uint8_t* bytes, size_t len, int Hb, int Wb) {
  P.Hb = Hb; P.Wb = Wb; P.Hbc = (Hb + 1) / 2; P.Wbc = (Wb + 1) / 2;
  const int runs_cap = Hb * Wb + 1;
  P.stream.resize(len + 8 * (size_t)runs_cap + 8);
  P.runs.resize((size_t)runs_cap);
  P.tables.resize(8);
  std::vector<int16_t> quant(192);
  std::vector<char> msg(128);
  memset(&P.p, 0, sizeof(P.p));
  P.p.stream = P.stream.data(); P.p.stream_cap = P.stream.size();
  P.p.runs = P.runs.data(); P.p.runs_cap = runs_cap;
  P.p.images = &P.image;
  P.p.tables = P.tables.data(); P.p.tables_cap = (int)P.tables.size();
  P.p.quant = quant.data();
  P.p.messages = msg.data(); P.p.message_len = (int)msg.size();
  P.p.threads = 1;
  const std::vector<uint8_t> copy(bytes, bytes + len);
  const uint8_t* bufs[1] = {copy.data()};
  const size_t lens[1] = {len};
  if (jpegscan::prepare(bufs, lens, 1, Hb, Wb, P.Hbc, P.Wbc, &P.p) < 0) fail("prepare: invalid arguments");
  if (P.image.status != 0 && !msg[0]) fail("a refusal without a message");
  if (P.image.status == 0) {
    P.stream.resize(P.p.stream_bytes);
    P.stream.shrink_to_fit();
  }
  P.p.stream = P.stream.data();
  P.p.quant = nullptr;
  P.p.messages = nullptr;
  return P.image.status;
}

// whole-grid outputs of one file, every element the sentinel
struct Grids {
  std::vector<int16_t> Y, C;
  explicit Grids(const Plan& P) : Y((size_t)P.Hb * P.Wb * 64, SENTINEL), C((size_t)2 * P.Hbc * P.Wbc * 64, SENTINEL) {}
  jpegwalk::Out out(const Plan& P) { return {1, P.Hb, P.Wb, P.Hbc, P.Wbc, Y.data(), C.data()}; }
};

// The one-lane reference walk of run r (jpegwalk::decode_run alone, as decode_kernel's lane does it).  *status: lowered to the error.
static void one_lane(const Plan& P, const jpegwalk::Out& g, const rgbnm_jpeg_run& r, int16_t* tile, int* status) {
  jpegwalk::Lane L;
  if (jpegwalk::check_run(r, &P.image, 1, P.p.stream_bytes, P.p.ntables, &L) != 0) fail("a run of the parser's fails check_run");
  const int err = jpegwalk::decode_run(P.stream.data(), r, L, P.tables.data(), jpegscan::ZIGZAG, g, tile);
  if (L.ncomp == 1) jpegwalk::zero_chroma_share(g, 0, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
  for (int k = 0; k < 64; ++k)
    if (tile[k]) fail("the tile is not zero after a run");
  if (err > 0) fail("a positive error code");
  if (err < *status) *status = err;
}
// ... of every run of the plan into G, which an accepted file leaves with no element unwritten, whatever its walk met.  Returns the status.
static int plain_walk(const Plan& P, Grids& G) {
  const jpegwalk::Out g = G.out(P);
  alignas(16) int16_t tile[64] = {0};
  int status = 0;
  for (int r = 0; r < P.p.nruns; ++r)
    if (P.runs[(size_t)r].nmcu) one_lane(P, g, P.runs[(size_t)r], tile, &status);
  for (int16_t v : G.Y)
    if (v == SENTINEL) fail("a luma element was never written");
  for (int16_t v : G.C)
    if (v == SENTINEL) fail("a chroma element was never written");
  return status;
}

enum Kind { AS_GIVEN, TRUNCATION, MUTATION };

// The input driver.  run(kind, file, bytes, len) -> status handles one input; a file as given must decode (status 0), one named
// *_refused.jpg must not.  Returns main's exit status.
template <class Run>
static int drive(int argc, char** argv, const char* prog, Run run) {
  std::vector<File> files;
  long share = 1;
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "--share" && i + 1 < argc) {
      share = atol(argv[++i]);
      if (share < 1) fail("--share needs a positive number");
      continue;
    }
    File f;
    f.name = argv[i];
    FILE* fp = fopen(argv[i], "rb");
    if (!fp) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), fp)) > 0) f.bytes.insert(f.bytes.end(), buf, buf + n);
    fclose(fp);
    if (!grid_of(f.bytes, &f.Hb, &f.Wb)) { fprintf(stderr, "%s: no frame header\n", argv[i]); return 2; }
    files.push_back(f);
  }
  if (files.size() < 2) { fprintf(stderr, "usage: %s [--share D] a.jpg b.jpg ...\n", prog); return 2; }
  for (const File& f : files) {
    const int st = run(AS_GIVEN, f, f.bytes.data(), f.bytes.size());
    if (f.refused() ? st == 0 : st != 0) {
      fprintf(stderr, "%s must %s as given\n", f.name.c_str(), f.refused() ? "be refused by the parser" : "decode");
      return 1;
    }
  }
  for (size_t k = 0; k < 2; ++k)
    for (size_t len = 0; len < files[k].bytes.size(); len += (size_t)share) run(TRUNCATION, files[k], files[k].bytes.data(), len);
  for (int k = 0; k < 6000; ++k) {
    const File& f = files[next() % files.size()];
    std::vector<uint8_t> b = f.bytes;
    // half of the mutations in the first 700 bytes (the marker segments), half anywhere (mostly the scan)
    const size_t at = (k & 1) ? next() % b.size() : next() % (b.size() < 700 ? b.size() : 700);
    b[at] = (k % 8 == 0) ? 0xFF : (uint8_t)next();
    if (k % share == 0) run(MUTATION, f, b.data(), b.size());
  }
  return 0;
}

}  // namespace jpegcheck
