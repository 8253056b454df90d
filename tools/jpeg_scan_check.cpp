// Stand-alone host check of the device JPEG decode's two halves on untrusted bytes: the marker parser (csrc/jpeg_scan.h) and the
// per-run Huffman walk (csrc/jpeg_walk.h: the very text the kernel runs, compiled here for the CPU).  Build it with the host
// sanitizers and give it JPEG files (tools/jpeg_scan_files.py writes the test suite's):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_scan_check.cpp -o jpeg_scan_check
//   ./jpeg_scan_check DIR/*.jpg
//
// It parses and decodes every file as given (that must succeed; a file named *_refused.jpg must be refused by the parser instead),
// then every truncation length of the first two, then 6000 single-byte mutations from a fixed seed.  Every outcome must be "decoded" or "refused with a status"; the outputs are heap blocks of the exact
// size, so a store outside them, like any read outside the file or the plan, stops the program.  Exit status 0: clean.
#define __host__
#define __device__
#include "../rgb-no-more_amd/csrc/jpeg_scan.h"
#include "../rgb-no-more_amd/csrc/jpeg_walk.h"

#include <cstdio>
#include <cstdlib>
#include <string>

struct File {
  std::string name;
  std::vector<uint8_t> bytes;
  int Hb = 0, Wb = 0;
};

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

struct Tally { long decoded = 0, refused_host = 0, refused_walk = 0; };

// one file through both halves; returns the status (0, host refusal or the walk's first error)
static int run_one(const uint8_t* bytes, size_t len, int Hb, int Wb, Tally* t, uint64_t* sum) {
  const int Hbc = (Hb + 1) / 2, Wbc = (Wb + 1) / 2;
  const int runs_cap = Hb * Wb + 1;
  // exact-size heap blocks: the sanitizer sees any access past them
  std::vector<uint8_t> stream(len + 8 * (size_t)runs_cap + 8);
  std::vector<rgbnm_jpeg_run> runs((size_t)runs_cap);
  std::vector<rgbnm_jpeg_hufftab> tables(8);
  std::vector<int16_t> quant(192), Y((size_t)Hb * Wb * 64, 0x5555), C((size_t)2 * Hbc * Wbc * 64, 0x5555);
  std::vector<char> msg(128);
  rgbnm_jpeg_image image;
  rgbnm_jpeg_plan p;
  memset(&p, 0, sizeof(p));
  p.stream = stream.data(); p.stream_cap = stream.size();
  p.runs = runs.data(); p.runs_cap = runs_cap;
  p.images = &image;
  p.tables = tables.data(); p.tables_cap = (int)tables.size();
  p.quant = quant.data();
  p.messages = msg.data(); p.message_len = (int)msg.size();
  p.threads = 1;
  std::vector<uint8_t> copy(bytes, bytes + len);              // exact size, too
  const uint8_t* bufs[1] = {copy.data()};
  const size_t lens[1] = {len};
  const int bad = jpegscan::prepare(bufs, lens, 1, Hb, Wb, Hbc, Wbc, &p);
  if (bad < 0) { fprintf(stderr, "prepare: invalid arguments\n"); exit(2); }
  if (image.status != 0) {
    if (!msg[0]) { fprintf(stderr, "a refusal without a message (status %d)\n", image.status); exit(2); }
    ++t->refused_host;
    return image.status;
  }
  jpegwalk::Out g = {1, Hb, Wb, Hbc, Wbc, Y.data(), C.data()};
  alignas(16) int16_t tile[64] = {0};
  int status = 0;
  for (int r = 0; r < p.nruns; ++r) {
    if (runs[(size_t)r].nmcu == 0) continue;
    jpegwalk::Lane L;
    int err = jpegwalk::check_run(runs[(size_t)r], &image, 1, p.stream_bytes, p.ntables, &L);
    if (!err) {
      err = jpegwalk::decode_run(stream.data(), runs[(size_t)r], L, tables.data(), jpegscan::ZIGZAG, g, tile);
      if (L.ncomp == 1) jpegwalk::zero_chroma_share(g, 0, (uint32_t)runs[(size_t)r].mcu0, (uint32_t)runs[(size_t)r].nmcu, L.total);
    }
    for (int k = 0; k < 64; ++k)
      if (tile[k]) { fprintf(stderr, "the tile is not zero after a run\n"); exit(2); }
    if (err && err < status) status = err;
    if (err && !status) status = err;
  }
  // an accepted file leaves no element unwritten, whatever its walk met
  for (int16_t v : Y)
    if (v == 0x5555) { fprintf(stderr, "a luma element was never written\n"); exit(2); }
  for (int16_t v : C)
    if (v == 0x5555) { fprintf(stderr, "a chroma element was never written\n"); exit(2); }
  for (int16_t v : Y) *sum = *sum * 1099511628211ull + (uint16_t)v;
  for (int16_t v : C) *sum = *sum * 1099511628211ull + (uint16_t)v;
  if (status) ++t->refused_walk; else ++t->decoded;
  return status;
}

int main(int argc, char** argv) {
  std::vector<File> files;
  for (int i = 1; i < argc; ++i) {
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
  if (files.size() < 2) { fprintf(stderr, "usage: jpeg_scan_check a.jpg b.jpg ...\n"); return 2; }
  Tally whole, cut, mut;
  uint64_t sum = 1469598103934665603ull;
  for (const File& f : files) {
    const int st = run_one(f.bytes.data(), f.bytes.size(), f.Hb, f.Wb, &whole, &sum);
    printf("%-28s %7zu bytes  grid %3d x %3d  status %d\n", f.name.c_str(), f.bytes.size(), f.Hb, f.Wb, st);
    const bool refuse = f.name.size() >= 12 && f.name.compare(f.name.size() - 12, 12, "_refused.jpg") == 0;
    if (refuse ? (st == 0 || whole.refused_walk) : st != 0) {
      fprintf(stderr, "%s must %s as given\n", f.name.c_str(), refuse ? "be refused by the parser" : "decode");
      return 1;
    }
  }
  for (size_t k = 0; k < 2; ++k)
    for (size_t len = 0; len < files[k].bytes.size(); ++len) run_one(files[k].bytes.data(), len, files[k].Hb, files[k].Wb, &cut, &sum);
  uint64_t s = 0x9E3779B97F4A7C15ull;                          // xorshift64, fixed seed
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  for (int k = 0; k < 6000; ++k) {
    const File& f = files[next() % files.size()];
    std::vector<uint8_t> b = f.bytes;
    // half of the mutations in the first 700 bytes (the marker segments), half anywhere (mostly the scan)
    const size_t at = (k & 1) ? next() % b.size() : next() % (b.size() < 700 ? b.size() : 700);
    b[at] = (k % 8 == 0) ? 0xFF : (uint8_t)next();
    run_one(b.data(), b.size(), f.Hb, f.Wb, &mut, &sum);
  }
  printf("as given:    %ld decoded, %ld refused by the parser, %ld by the walk\n", whole.decoded, whole.refused_host, whole.refused_walk);
  printf("truncations: %ld decoded, %ld refused by the parser, %ld by the walk\n", cut.decoded, cut.refused_host, cut.refused_walk);
  printf("mutations:   %ld decoded, %ld refused by the parser, %ld by the walk\n", mut.decoded, mut.refused_host, mut.refused_walk);
  printf("checksum %016llx\n", (unsigned long long)sum);
  return 0;
}
