// Stand-alone host check of the device JPEG decode's SPLIT path on untrusted bytes (csrc/jpeg_split.h: the very text the segment
// lanes run, compiled here for the CPU).  The lanes are emulated one after another, pass by pass -- map, scout, `rounds` sync rounds
// on double-buffered exits, verify, write, then the one-lane walk for what is left -- and for every input the outputs, the status and
// the path are compared with what jpegwalk::decode_run alone gives on the same plan.  Build it with the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_split_check.cpp -o jpeg_split_check
//   ./jpeg_split_check [--share D] DIR/*.jpg          (tools/jpeg_scan_files.py writes the test suite's files)
//
// Inputs (the driver of jpeg_check_common.h): every file as given, every truncation length of the first two, 6000 single-byte
// mutations from a fixed seed (--share D: every D-th truncation and mutation only).  Each goes through seg_bits 256 (runs of at least 16 segments are split, the default)
// and 2048 (at least 2, so that files of a few KB are split at all), each with rounds 0, 2 and 64.  The outputs are heap blocks of
// the exact size, and so are the scratch records.  Exit status 0: clean, and every output, status and path as expected:
//   path 0 where no run is split; else 1 or 2, and 2 wherever the one-lane walk of a split run ends in an error.
#include "jpeg_check_common.h"
#include "../rgb-no-more_amd/csrc/jpeg_split.h"

using namespace jpegcheck;

struct Result {
  std::vector<int16_t> Y, C;
  int status = 0, path = 0;
};

struct Count { long walks = 0, segs = 0; };

static Result split(const Plan& P, int Hb, int Wb, int seg_bits, int min_seg, int rounds, Count* cnt) {
  using namespace jpegsplit;
  const int Hbc = (Hb + 1) / 2, Wbc = (Wb + 1) / 2, nruns = P.p.nruns;
  Result R;
  R.Y.assign((size_t)Hb * Wb * 64, SENTINEL);
  R.C.assign((size_t)2 * Hbc * Wbc * 64, SENTINEL);
  jpegwalk::Out g = {1, Hb, Wb, Hbc, Wbc, R.Y.data(), R.C.data()};
  const size_t bytes = scratch_bytes(P.p.stream_bytes, nruns, seg_bits);
  if (!bytes) fail("scratch_bytes refused the plan");
  std::vector<uint64_t> mem((bytes + 7) / 8);                 // exact size (rounded to 8): the sanitizer sees any access past it
  Scratch s = carve(mem.data(), P.p.stream_bytes, nruns, seg_bits);
  const uint8_t* stream = P.stream.data();
  const rgbnm_jpeg_hufftab* tabs = P.tables.data();
  alignas(16) int16_t tile[64] = {0};
  // init, map
  for (uint32_t i = 0; i < s.nslots; ++i) s.seg_run[i] = -1;
  std::vector<Lane> lanes((size_t)nruns);
  for (int ri = 0; ri < nruns; ++ri) {
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    RunInfo info = {0u, 0u};
    if (r.nmcu != 0 && jpegwalk::check_run(r, &P.image, 1, P.p.stream_bytes, P.p.ntables, &lanes[(size_t)ri]) == 0)
      info = map_run(r, ri, seg_bits, min_seg, s.nslots);
    s.info[ri] = info;
    if (info.nseg && R.path < 1) R.path = 1;
    for (uint32_t j = 0; j < info.nseg; ++j) {
      if (s.seg_run[info.base + j] != -1) fail("two runs share a slot");
      s.seg_run[info.base + j] = ri;
    }
  }
  // a segment lane's view of its slot, exactly as the kernel derives it
  auto lane_of = [&](uint32_t slot, int* ri, uint32_t* j) {
    *ri = s.seg_run[slot];
    if (*ri < 0 || *ri >= nruns) return false;
    *j = slot - s.info[*ri].base;
    return *j < s.info[*ri].nseg;
  };
  // scout
  for (uint32_t slot = 0; slot < s.nslots; ++slot) {
    int ri;
    uint32_t j;
    if (!lane_of(slot, &ri, &j)) continue;
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    const uint64_t state = j == 0 ? pack_state(0, 0, 0) : seg_first_state(j, seg_bits);
    s.entry[slot] = state;
    s.exits[0][slot] = scout_walk(stream, r, lanes[(size_t)ri], tabs, state, seg_end(r, j, seg_bits), (uint32_t)seg_bits + 1u, &s.rec[slot]);
    ++cnt->walks;
    ++cnt->segs;
  }
  // sync rounds
  for (int round = 0; round < rounds; ++round) {
    const int cur = round & 1, nxt = cur ^ 1;
    for (uint32_t slot = 0; slot < s.nslots; ++slot) {
      int ri;
      uint32_t j;
      if (!lane_of(slot, &ri, &j)) continue;
      const uint64_t mine = s.exits[cur][slot], pe = j ? s.exits[cur][slot - 1] : 0;
      if (j == 0 || s.entry[slot] == pe) {
        s.exits[nxt][slot] = mine;
        continue;
      }
      const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
      s.entry[slot] = pe;
      s.exits[nxt][slot] = scout_walk(stream, r, lanes[(size_t)ri], tabs, pe, seg_end(r, j, seg_bits), (uint32_t)seg_bits + 1u, &s.rec[slot]);
      ++cnt->walks;
    }
  }
  // verify and scan
  const uint64_t* fin = s.exits[rounds & 1];
  for (int ri = 0; ri < nruns; ++ri) {
    const RunInfo info = s.info[ri];
    if (!info.nseg) continue;
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    const uint64_t N = (uint64_t)r.nmcu * (uint64_t)lanes[(size_t)ri].nblk;
    uint32_t carry[5] = {0, 0, 0, 0, 0};
    bool bad = false, found = false;
    for (uint32_t j = 0; j < info.nseg; ++j) {
      const uint32_t slot = info.base + j;
      const SegRec& c = s.rec[slot];
      if (s.seg_run[slot] != ri || s.entry[slot] != (j ? fin[slot - 1] : pack_state(0, 0, 0))) bad = true;
      const int verdict = seg_verdict(c, carry[0], N, r.nbytes * 8u);
      bad = bad || verdict == 1;
      found = found || verdict == 2;
      s.scan[slot].b0 = carry[1];
      for (int q = 0; q < 3; ++q) s.scan[slot].p[q] = carry[2 + q];
      carry[0] += c.ndone;
      carry[1] += c.nstart;
      for (int q = 0; q < 3; ++q) carry[2 + q] += c.dc[q];
    }
    if (bad || !found) R.path = 2;
  }
  // write
  if (R.path == 1) {
    for (uint32_t slot = 0; slot < s.nslots; ++slot) {
      int ri;
      uint32_t j;
      if (!lane_of(slot, &ri, &j)) continue;
      const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
      const Lane& L = lanes[(size_t)ri];
      if (write_walk(stream, r, L, tabs, jpegscan::ZIGZAG, g, tile, s.entry[slot], seg_end(r, j, seg_bits), (uint32_t)seg_bits + 64u,
                     s.scan[slot]) != 0)
        fail("the write walk met what verify should have excluded");
      if (L.ncomp == 1) zero_chroma_part(g, 0, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total, j, s.info[ri].nseg);
      for (int k = 0; k < 64; ++k)
        if (tile[k]) fail("the tile is not zero after a segment");
    }
  }
  // path 1 claims that the one-lane walk of every split run ends without an error
  if (R.path == 1) {
    Result scrap = R;
    jpegwalk::Out gs = {1, Hb, Wb, Hbc, Wbc, scrap.Y.data(), scrap.C.data()};
    for (int ri = 0; ri < nruns; ++ri)
      if (s.info[ri].nseg && jpegwalk::decode_run(stream, P.runs[(size_t)ri], lanes[(size_t)ri], tabs, jpegscan::ZIGZAG, gs, tile) != 0)
        fail("path 1 for a run whose one-lane walk ends in an error");
  }
  // what is left
  for (int ri = 0; ri < nruns; ++ri) {
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    if (r.nmcu == 0 || (s.info[ri].nseg && R.path == 1)) continue;
    one_lane(P, g, r, tile, &R.status);
  }
  return R;
}

struct Tally { long decoded = 0, refused_host = 0, refused_walk = 0, path[3] = {0, 0, 0}; };
static Count g_count;

static int run_one(const uint8_t* bytes, size_t len, int Hb, int Wb, Tally* t) {
  Plan P;
  if (const int st = prepare(P, bytes, len, Hb, Wb)) {
    ++t->refused_host;
    return st;
  }
  Grids want(P);
  const int want_status = plain_walk(P, want);
  const int cfg[2][2] = {{256, jpegsplit::MIN_SEG}, {2048, 2}};
  const int rounds[3] = {0, 2, 64};
  for (int c = 0; c < 2; ++c)
    for (int q = 0; q < 3; ++q) {
      const Result got = split(P, Hb, Wb, cfg[c][0], cfg[c][1], rounds[q], &g_count);
      if (got.Y != want.Y || got.C != want.C) fail("the split decode's output differs from the one-lane walk's");
      if (got.status != want_status) fail("the split decode's status differs from the one-lane walk's");
      ++t->path[got.path];
    }
  if (want_status) ++t->refused_walk; else ++t->decoded;
  return want_status;
}

int main(int argc, char** argv) {
  Tally tally[3];                                               // as given, truncations, mutations
  const int rc = drive(argc, argv, "jpeg_split_check", [&](Kind kind, const File& f, const uint8_t* bytes, size_t len) {
    const long before = tally[kind].path[2];
    const int st = run_one(bytes, len, f.Hb, f.Wb, &tally[kind]);
    if (kind == AS_GIVEN) {
      if (tally[AS_GIVEN].refused_walk) fail("a file as given got as far as the walk and was refused there");
      printf("%-36s %7zu bytes  status %d  fallbacks in 6 configurations: %ld\n", f.name.c_str(), len, st, tally[kind].path[2] - before);
    }
    return st;
  });
  if (rc) return rc;
  const char* names[3] = {"as given:   ", "truncations:", "mutations:  "};
  for (int i = 0; i < 3; ++i)
    printf("%s %ld decoded, %ld refused by the parser, %ld by the walk; per configuration: %ld not split, %ld split, %ld split then one-lane\n",
           names[i], tally[i].decoded, tally[i].refused_host, tally[i].refused_walk, tally[i].path[0], tally[i].path[1], tally[i].path[2]);
  printf("segment walks per segment: %.2f (%ld walks, %ld segments)\n", g_count.segs ? (double)g_count.walks / (double)g_count.segs : 0.0,
         g_count.walks, g_count.segs);
  return 0;
}
