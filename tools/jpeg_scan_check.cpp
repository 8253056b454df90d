// Stand-alone host check of the device JPEG decode's two halves on untrusted bytes: the marker parser (csrc/jpeg_scan.h) and the
// per-run Huffman walk (csrc/jpeg_walk.h: the very text the kernel runs, compiled here for the CPU).  Build it with the host
// sanitizers and give it JPEG files (tools/jpeg_scan_files.py writes the test suite's):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_scan_check.cpp -o jpeg_scan_check
//   ./jpeg_scan_check [--share D] DIR/*.jpg
//
// It parses and decodes every file as given (that must succeed; a file named *_refused.jpg must be refused by the parser instead),
// then every truncation length of the first two, then 6000 single-byte mutations from a fixed seed (jpeg_check_common.h has the
// driver).  Every outcome must be "decoded" or "refused with a status"; the outputs are heap blocks of the exact size, so a store
// outside them, like any read outside the file or the plan, stops the program.  The checksum over every output makes two builds of
// the walk comparable.  Exit status 0: clean; 1: a check failed (the shared fail(), also where this program used to exit with 2);
// 2: bad arguments or an unreadable file.
#include "jpeg_check_common.h"

using namespace jpegcheck;

struct Tally { long decoded = 0, refused_host = 0, refused_walk = 0; };

// one input through both halves; returns the status (0, host refusal or the walk's first error)
static int run_one(const uint8_t* bytes, size_t len, int Hb, int Wb, Tally* t, uint64_t* sum) {
  Plan P;
  if (const int st = prepare(P, bytes, len, Hb, Wb)) {
    ++t->refused_host;
    return st;
  }
  Grids G(P);
  const int status = plain_walk(P, G);
  for (int16_t v : G.Y) *sum = *sum * 1099511628211ull + (uint16_t)v;
  for (int16_t v : G.C) *sum = *sum * 1099511628211ull + (uint16_t)v;
  if (status) ++t->refused_walk; else ++t->decoded;
  return status;
}

int main(int argc, char** argv) {
  Tally tally[3];                                               // as given, truncations, mutations
  uint64_t sum = 1469598103934665603ull;
  const int rc = drive(argc, argv, "jpeg_scan_check", [&](Kind kind, const File& f, const uint8_t* bytes, size_t len) {
    const int st = run_one(bytes, len, f.Hb, f.Wb, &tally[kind], &sum);
    if (kind == AS_GIVEN) {
      printf("%-28s %7zu bytes  grid %3d x %3d  status %d\n", f.name.c_str(), len, f.Hb, f.Wb, st);
      if (tally[AS_GIVEN].refused_walk) fail("a file as given got as far as the walk and was refused there");
    }
    return st;
  });
  if (rc) return rc;
  const char* names[3] = {"as given:   ", "truncations:", "mutations:  "};
  for (int i = 0; i < 3; ++i)
    printf("%s %ld decoded, %ld refused by the parser, %ld by the walk\n", names[i], tally[i].decoded, tally[i].refused_host, tally[i].refused_walk);
  printf("checksum %016llx\n", (unsigned long long)sum);
  return 0;
}
