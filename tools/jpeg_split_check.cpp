// Stand-alone host check of the device JPEG decode's SPLIT path on untrusted bytes (csrc/jpeg_split.h: the very text the segment
// lanes run, compiled here for the CPU).  The lanes are emulated one after another, pass by pass -- map, scout, `rounds` sync rounds
// on double-buffered exits, verify, write, then the one-lane walk for what is left -- and for every input the outputs, the status and
// the path are compared with what jpegwalk::decode_run alone gives on the same plan.  Build it with the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_split_check.cpp -o jpeg_split_check
//   ./jpeg_split_check [--share D] DIR/*.jpg          (tools/jpeg_scan_files.py writes the test suite's files)
//
// Inputs: every file as given, every truncation length of the first two, 6000 single-byte mutations from a fixed seed (--share D:
// every D-th truncation and mutation only).  Each goes through seg_bits 256 (runs of at least 16 segments are split, the default)
// and 2048 (at least 2, so that files of a few KB are split at all), each with rounds 0, 2 and 64.  The outputs are heap blocks of
// the exact size, and so are the scratch records.  Exit status 0: clean, and every output, status and path as expected:
//   path 0 where no run is split; else 1 or 2, and 2 wherever the one-lane walk of a split run ends in an error.
#define __host__
#define __device__
#include "../rgb-no-more_amd/csrc/jpeg_scan.h"
#include "../rgb-no-more_amd/csrc/jpeg_walk.h"
#include "../rgb-no-more_amd/csrc/jpeg_split.h"

#include <cstdio>
#include <cstdlib>
#include <string>

struct File {
  std::string name;
  std::vector<uint8_t> bytes;
  int Hb = 0, Wb = 0;
};

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

struct Plan {
  std::vector<uint8_t> stream;
  std::vector<rgbnm_jpeg_run> runs;
  std::vector<rgbnm_jpeg_hufftab> tables;
  rgbnm_jpeg_image image;
  rgbnm_jpeg_plan p;
};

struct Result {
  std::vector<int16_t> Y, C;
  int status = 0, path = 0;
};

static void fail(const char* what) {
  fprintf(stderr, "%s\n", what);
  exit(1);
}

static void one_lane(const Plan& P, const jpegwalk::Out& g, const rgbnm_jpeg_run& r, int16_t* tile, int* status) {
  jpegwalk::Lane L;
  int err = jpegwalk::check_run(r, &P.image, 1, P.p.stream_bytes, P.p.ntables, &L);
  if (!err) {
    err = jpegwalk::decode_run(P.stream.data(), r, L, P.tables.data(), jpegscan::ZIGZAG, g, tile);
    if (L.ncomp == 1) jpegwalk::zero_chroma_share(g, 0, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
  }
  for (int k = 0; k < 64; ++k)
    if (tile[k]) fail("the tile is not zero after a run");
  if (err && err < *status) *status = err;
}

static Result plain(const Plan& P, int Hb, int Wb) {
  const int Hbc = (Hb + 1) / 2, Wbc = (Wb + 1) / 2;
  Result R;
  R.Y.assign((size_t)Hb * Wb * 64, 0x5555);
  R.C.assign((size_t)2 * Hbc * Wbc * 64, 0x5555);
  jpegwalk::Out g = {1, Hb, Wb, Hbc, Wbc, R.Y.data(), R.C.data()};
  alignas(16) int16_t tile[64] = {0};
  for (int r = 0; r < P.p.nruns; ++r)
    if (P.runs[(size_t)r].nmcu) one_lane(P, g, P.runs[(size_t)r], tile, &R.status);
  return R;
}

struct Count { long walks = 0, segs = 0; };

static Result split(const Plan& P, int Hb, int Wb, int seg_bits, int min_seg, int rounds, Count* cnt) {
  using namespace jpegsplit;
  const int Hbc = (Hb + 1) / 2, Wbc = (Wb + 1) / 2, nruns = P.p.nruns;
  Result R;
  R.Y.assign((size_t)Hb * Wb * 64, 0x5555);
  R.C.assign((size_t)2 * Hbc * Wbc * 64, 0x5555);
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
  const int Hbc = (Hb + 1) / 2, Wbc = (Wb + 1) / 2, runs_cap = Hb * Wb + 1;
  Plan P;
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
  std::vector<uint8_t> copy(bytes, bytes + len);
  const uint8_t* bufs[1] = {copy.data()};
  const size_t lens[1] = {len};
  if (jpegscan::prepare(bufs, lens, 1, Hb, Wb, Hbc, Wbc, &P.p) < 0) fail("prepare: invalid arguments");
  if (P.image.status != 0) {
    ++t->refused_host;
    return P.image.status;
  }
  P.stream.resize(P.p.stream_bytes);                          // the used prefix alone, as the device holds it
  P.stream.shrink_to_fit();
  const Result want = plain(P, Hb, Wb);
  for (int16_t v : want.Y)
    if (v == 0x5555) fail("a luma element was never written");
  for (int16_t v : want.C)
    if (v == 0x5555) fail("a chroma element was never written");
  const int cfg[2][2] = {{256, jpegsplit::MIN_SEG}, {2048, 2}};
  const int rounds[3] = {0, 2, 64};
  for (int c = 0; c < 2; ++c)
    for (int q = 0; q < 3; ++q) {
      const Result got = split(P, Hb, Wb, cfg[c][0], cfg[c][1], rounds[q], &g_count);
      if (got.Y != want.Y || got.C != want.C) fail("the split decode's output differs from the one-lane walk's");
      if (got.status != want.status) fail("the split decode's status differs from the one-lane walk's");
      ++t->path[got.path];
    }
  if (want.status) ++t->refused_walk; else ++t->decoded;
  return want.status;
}

int main(int argc, char** argv) {
  std::vector<File> files;
  int share = 1;
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "--share" && i + 1 < argc) {
      share = atoi(argv[++i]);
      if (share < 1) share = 1;
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
  if (files.size() < 2) { fprintf(stderr, "usage: jpeg_split_check [--share D] a.jpg b.jpg ...\n"); return 2; }
  Tally whole, cut, mut;
  for (const File& f : files) {
    const long before = whole.path[2];
    const int st = run_one(f.bytes.data(), f.bytes.size(), f.Hb, f.Wb, &whole);
    const bool refuse = f.name.size() >= 12 && f.name.compare(f.name.size() - 12, 12, "_refused.jpg") == 0;
    if (refuse ? (st == 0 || whole.refused_walk) : st != 0) {
      fprintf(stderr, "%s must %s as given\n", f.name.c_str(), refuse ? "be refused by the parser" : "decode");
      return 1;
    }
    printf("%-36s %7zu bytes  status %d  fallbacks in 6 configurations: %ld\n", f.name.c_str(), f.bytes.size(), st, whole.path[2] - before);
  }
  for (size_t k = 0; k < 2; ++k)
    for (size_t len = 0; len < files[k].bytes.size(); len += (size_t)share) run_one(files[k].bytes.data(), len, files[k].Hb, files[k].Wb, &cut);
  uint64_t s = 0x9E3779B97F4A7C15ull;                          // xorshift64, fixed seed
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  for (int k = 0; k < 6000; ++k) {
    const File& f = files[next() % files.size()];
    std::vector<uint8_t> b = f.bytes;
    const size_t at = (k & 1) ? next() % b.size() : next() % (b.size() < 700 ? b.size() : 700);
    b[at] = (k % 8 == 0) ? 0xFF : (uint8_t)next();
    if (k % share == 0) run_one(b.data(), b.size(), f.Hb, f.Wb, &mut);
  }
  const Tally* ts[3] = {&whole, &cut, &mut};
  const char* names[3] = {"as given:   ", "truncations:", "mutations:  "};
  for (int i = 0; i < 3; ++i)
    printf("%s %ld decoded, %ld refused by the parser, %ld by the walk; per configuration: %ld not split, %ld split, %ld split then one-lane\n",
           names[i], ts[i]->decoded, ts[i]->refused_host, ts[i]->refused_walk, ts[i]->path[0], ts[i]->path[1], ts[i]->path[2]);
  printf("segment walks per segment: %.2f (%ld walks, %ld segments)\n", g_count.segs ? (double)g_count.walks / (double)g_count.segs : 0.0,
         g_count.walks, g_count.segs);
  return 0;
}
