// Stand-alone host check of the device JPEG decode's CROP form on untrusted bytes (csrc/jpeg_walk.h: check_box, crop_mcus,
// decode_run_crop, zero_chroma_share_crop -- the very text the lanes of rgbnm_jpeg_decode_batch_crop run, compiled here for the CPU).
// For every input and every box it runs the plain walk and the crop walk of every run and compares.  Build it with the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_crop_check.cpp -o jpeg_crop_check
//   ./jpeg_crop_check [--share D] DIR/*.jpg          (tools/jpeg_scan_files.py writes the test suite's files)
//
// Inputs: every file as given with the largest even box and BOXES_GIVEN boxes from a fixed seed, then every truncation length of the
// first two files and 6000 single-byte mutations, each with BOXES_DAMAGED boxes (--share D: every D-th truncation and mutation only).
// For every input that the parser accepts and every box:
//   (a) the packed crops equal the box cut out of the plain walk's whole-grid output, every element of them written;
//   (b) status_whole <= status_crop <= 0;      (c) status_crop == 0 wherever status_whole == 0;
//   the MCUs walked per run equal a brute-force count (up to the last MCU of the run with a block inside its component's box), so a
//   run without such an MCU is not walked at all; the guard bands around both packed slots are untouched; the tile is zero after a run.
// A box that is odd, outside the grid or whose offset does not fit must be refused with RGBNM_JPEG_EBOX before anything is written.
// The packed buffers are heap blocks of the exact size.  Exit status 0: clean.
#define __host__
#define __device__
#include "../rgb-no-more_amd/csrc/jpeg_scan.h"
#include "../rgb-no-more_amd/csrc/jpeg_walk.h"

#include <cstdio>
#include <cstdlib>
#include <string>

static const int BOXES_GIVEN = 12, BOXES_DAMAGED = 2, GUARD = 64;
static const int16_t SENTINEL = 0x5555;

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

static void fail(const char* what) {
  fprintf(stderr, "%s\n", what);
  exit(1);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;             // xorshift64, fixed seed
static uint64_t next() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

struct Tally {
  long decoded = 0, refused_host = 0, refused_walk = 0;        // inputs, by the plain walk's verdict
  long boxes = 0, crop_clean = 0;                              // boxes tried; of them, status_crop == 0
  long hidden = 0;                                             // ... while status_whole < 0: the error lay behind the last needed MCU
  long runs = 0, skipped = 0, early = 0;                       // runs seen by a box; not walked; stopped before their end
  long long mcus = 0, walked = 0;
};

struct Plan {
  std::vector<uint8_t> stream;
  std::vector<rgbnm_jpeg_run> runs;
  std::vector<rgbnm_jpeg_hufftab> tables;
  rgbnm_jpeg_image image;
  rgbnm_jpeg_plan p;
};

// MCUs of the run up to the last one with a block inside its component's box: by looking at every block of every MCU
static uint32_t brute_walked(const rgbnm_jpeg_run& r, const rgbnm_jpeg_image& im, const int* box) {
  int last = -1;
  for (int m = r.mcu0; m < r.mcu0 + r.nmcu; ++m) {
    const int mx = m % im.mcus_x, my = m / im.mcus_x;
    for (int b = 0; b < im.nblk; ++b) {
      const int c = im.blk_comp[b], bx = mx * im.hs[c] + im.blk_dx[b], by = my * im.vs[c] + im.blk_dy[b];
      const int t = c ? box[0] / 2 : box[0], l = c ? box[1] / 2 : box[1], h = c ? box[2] / 2 : box[2], w = c ? box[3] / 2 : box[3];
      if (by >= t && by < t + h && bx >= l && bx < l + w) last = m;
    }
  }
  return last < 0 ? 0u : (uint32_t)(last - r.mcu0 + 1);
}

// one box on a prepared plan against the plain walk's result
static void one_box(Plan& P, int Hb, int Wb, const int* box, const std::vector<int16_t>& Y, const std::vector<int16_t>& C, int status_whole,
                    Tally* t) {
  const int Hbc = (Hb + 1) / 2, Wbc = (Wb + 1) / 2;
  const size_t ny = (size_t)64 * box[2] * box[3], nc = (size_t)128 * (box[2] / 2) * (box[3] / 2);
  const long long y_off = GUARD + 8 * (long long)(next() % 5), c_off = GUARD + 8 * (long long)(next() % 5);
  std::vector<int16_t> Yp((size_t)y_off + ny + GUARD, SENTINEL), Cp((size_t)c_off + nc + GUARD, SENTINEL);
  alignas(16) int16_t tile[64] = {0};
  int status = 0;
  ++t->boxes;
  for (int ri = 0; ri < P.p.nruns; ++ri) {
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    if (r.nmcu == 0) continue;
    jpegwalk::Lane L;
    jpegwalk::Crop B;
    if (jpegwalk::check_run(r, &P.image, 1, P.p.stream_bytes, P.p.ntables, &L) != 0) fail("a run of the parser's fails check_run");
    // the buffers end exactly behind the slots' guard bands: y_elems / c_elems are their sizes
    if (jpegwalk::check_box(box, y_off, c_off, Hb, Wb, Hbc, Wbc, Yp.data(), Yp.size(), Cp.data(), Cp.size(), &B) != 0)
      fail("a valid box was refused");
    const uint32_t nwalk = jpegwalk::crop_mcus(r, L, B);
    if (nwalk != brute_walked(r, P.image, box)) fail("crop_mcus differs from the brute-force count");
    ++t->runs;
    t->mcus += r.nmcu;
    t->walked += nwalk;
    if (nwalk == 0) ++t->skipped;
    else if (nwalk < (uint32_t)r.nmcu) ++t->early;
    int err = 0;
    if (nwalk) err = jpegwalk::decode_run_crop(P.stream.data(), r, L, P.tables.data(), jpegscan::ZIGZAG, B, nwalk, tile);
    if (L.ncomp == 1) jpegwalk::zero_chroma_share_crop(B, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
    for (int k = 0; k < 64; ++k)
      if (tile[k]) fail("the tile is not zero after a crop run");
    if (err > 0) fail("a positive error code");
    if (err < status) status = err;
  }
  // guards
  for (size_t i = 0; i < Yp.size(); ++i)
    if ((i < (size_t)y_off || i >= (size_t)y_off + ny) && Yp[i] != SENTINEL) fail("a luma guard element changed");
  for (size_t i = 0; i < Cp.size(); ++i)
    if ((i < (size_t)c_off || i >= (size_t)c_off + nc) && Cp[i] != SENTINEL) fail("a chroma guard element changed");
  // (a)
  for (int y = 0; y < box[2]; ++y)
    for (int x = 0; x < box[3]; ++x)
      if (memcmp(&Yp[(size_t)y_off + ((size_t)y * box[3] + x) * 64], &Y[((size_t)(box[0] + y) * Wb + (box[1] + x)) * 64], 128))
        fail("a luma block of the crop differs from the whole-grid decode");
  const int hc = box[2] / 2, wc = box[3] / 2;
  for (int c = 0; c < 2; ++c)
    for (int y = 0; y < hc; ++y)
      for (int x = 0; x < wc; ++x)
        if (memcmp(&Cp[(size_t)c_off + (((size_t)c * hc + y) * wc + x) * 64],
                   &C[(((size_t)c * Hbc + (box[0] / 2 + y)) * Wbc + (box[1] / 2 + x)) * 64], 128))
          fail("a chroma block of the crop differs from the whole-grid decode");
  // (b), (c)
  if (!(status_whole <= status && status <= 0)) fail("status_whole <= status_crop <= 0 does not hold");
  if (status_whole == 0 && status != 0) fail("the crop decode fails a file the whole decode accepts");
  if (status == 0) ++t->crop_clean;
  if (status == 0 && status_whole != 0) ++t->hidden;
}

// boxes the walk must refuse, with nothing written
static void bad_boxes(int Hb, int Wb) {
  const int Hbc = (Hb + 1) / 2, Wbc = (Wb + 1) / 2, he = Hb & ~1, we = Wb & ~1;
  std::vector<int16_t> Yp((size_t)64 * Hb * Wb + 8), Cp((size_t)128 * Hbc * Wbc + 8);
  jpegwalk::Crop B;
  auto refused = [&](int t, int l, int h, int w, long long yo, long long co, size_t ye, size_t ce) {
    const int box[4] = {t, l, h, w};
    return jpegwalk::check_box(box, yo, co, Hb, Wb, Hbc, Wbc, Yp.data(), ye, Cp.data(), ce, &B) == RGBNM_JPEG_EBOX;
  };
  const size_t ye = Yp.size(), ce = Cp.size();
  bool ok = refused(0, 0, Hb + 2 - (Hb & 1), 2, 0, 0, ye, ce) && refused(0, 0, 2, Wb + 2 - (Wb & 1), 0, 0, ye, ce) &&
            refused(-2, 0, 2, 2, 0, 0, ye, ce) && refused(0, -2, 2, 2, 0, 0, ye, ce) && refused(0, 0, 0, 2, 0, 0, ye, ce) &&
            refused(0, 0, 2, 0, 0, 0, ye, ce) && refused(0, 0, -2, 2, 0, 0, ye, ce) && refused(1, 0, 2, 2, 0, 0, ye, ce) &&
            refused(0, 1, 2, 2, 0, 0, ye, ce) && refused(0, 0, 1, 2, 0, 0, ye, ce) && refused(0, 0, 2, 1, 0, 0, ye, ce) &&
            refused(0x7FFFFFFE, 0, 2, 2, 0, 0, ye, ce) && refused(0, 0, 0x7FFFFFFE, 2, 0, 0, ye, ce) && refused(2, 0, 0x7FFFFFFE, 2, 0, 0, ye, ce);
  if (he >= 2 && we >= 2) {
    const size_t ny = (size_t)64 * he * we, nc = (size_t)128 * (he / 2) * (we / 2);
    jpegwalk::Crop G;
    const int box[4] = {0, 0, he, we};
    if (jpegwalk::check_box(box, 8, 8, Hb, Wb, Hbc, Wbc, Yp.data(), ny + 8, Cp.data(), nc + 8, &G) != 0) fail("the largest box was refused");
    ok = ok && refused(0, 0, he, we, 8, 8, ny + 7, nc + 8) && refused(0, 0, he, we, 8, 8, ny + 8, nc + 7) &&
         refused(0, 0, he, we, 4, 0, ye, ce) && refused(0, 0, he, we, 0, 4, ye, ce) && refused(0, 0, he, we, -8, 0, ye, ce) &&
         refused(0, 0, he, we, 0, -8, ye, ce) && refused(0, 0, he, we, (long long)1 << 62, 0, ye, ce) &&
         refused(0, 0, he, we, 0, (long long)0x7FFFFFFFFFFFFFF8ll, ye, ce) && refused(he, 0, 2, 2, 0, 0, ye, ce) &&
         refused(0, we, 2, 2, 0, 0, ye, ce);
  }
  if (!ok) fail("a bad box or offset was accepted");
}

// one input: the plain walk, then the crop walk for `nbox` boxes (and the largest one if `largest`)
static int run_one(const uint8_t* bytes, size_t len, int Hb, int Wb, int nbox, bool largest, Tally* t) {
  const int Hbc = (Hb + 1) / 2, Wbc = (Wb + 1) / 2;
  const int runs_cap = Hb * Wb + 1;
  Plan P;
  P.stream.resize(len + 8 * (size_t)runs_cap + 8);
  P.runs.resize((size_t)runs_cap);
  P.tables.resize(8);
  std::vector<int16_t> quant(192), Y((size_t)Hb * Wb * 64, SENTINEL), C((size_t)2 * Hbc * Wbc * 64, SENTINEL);
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
  jpegwalk::Out g = {1, Hb, Wb, Hbc, Wbc, Y.data(), C.data()};
  alignas(16) int16_t tile[64] = {0};
  int status = 0;
  for (int ri = 0; ri < P.p.nruns; ++ri) {
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    if (r.nmcu == 0) continue;
    jpegwalk::Lane L;
    if (jpegwalk::check_run(r, &P.image, 1, P.p.stream_bytes, P.p.ntables, &L) != 0) fail("a run of the parser's fails check_run");
    const int err = jpegwalk::decode_run(P.stream.data(), r, L, P.tables.data(), jpegscan::ZIGZAG, g, tile);
    if (L.ncomp == 1) jpegwalk::zero_chroma_share(g, 0, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
    if (err < status) status = err;
  }
  if (status) ++t->refused_walk; else ++t->decoded;
  const int he = Hb & ~1, we = Wb & ~1;
  if (he < 2 || we < 2) return status;                          // no even box fits this grid
  if (largest) {
    const int box[4] = {0, 0, he, we};
    one_box(P, Hb, Wb, box, Y, C, status, t);
  }
  for (int k = 0; k < nbox; ++k) {
    int box[4];
    box[2] = 2 * (1 + (int)(next() % (uint64_t)(he / 2)));
    box[3] = 2 * (1 + (int)(next() % (uint64_t)(we / 2)));
    if (k % 3 == 0) box[2] = box[2] > 4 ? 2 : box[2], box[3] = box[3] > 4 ? 2 : box[3];     // small boxes skip the most
    box[0] = 2 * (int)(next() % (uint64_t)((he - box[2]) / 2 + 1));
    box[1] = 2 * (int)(next() % (uint64_t)((we - box[3]) / 2 + 1));
    one_box(P, Hb, Wb, box, Y, C, status, t);
  }
  return status;
}

static void report(const char* what, const Tally& t) {
  printf("%-12s %ld decoded, %ld refused by the parser, %ld by the walk; %ld boxes: %ld clean (%ld of them hide a later error), "
         "%ld runs: %ld skipped, %ld stopped early, %lld of %lld MCUs walked\n",
         what, t.decoded, t.refused_host, t.refused_walk, t.boxes, t.crop_clean, t.hidden, t.runs, t.skipped, t.early, t.walked, t.mcus);
}

int main(int argc, char** argv) {
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
  if (files.size() < 2) { fprintf(stderr, "usage: jpeg_crop_check [--share D] a.jpg b.jpg ...\n"); return 2; }
  Tally whole, cut, mut;
  for (const File& f : files) {
    bad_boxes(f.Hb, f.Wb);
    const int st = run_one(f.bytes.data(), f.bytes.size(), f.Hb, f.Wb, BOXES_GIVEN, true, &whole);
    const bool refuse = f.name.size() >= 12 && f.name.compare(f.name.size() - 12, 12, "_refused.jpg") == 0;
    if (refuse ? st == 0 : st != 0) {
      fprintf(stderr, "%s must %s as given\n", f.name.c_str(), refuse ? "be refused by the parser" : "decode");
      return 1;
    }
  }
  if (whole.crop_clean != whole.boxes || whole.skipped == 0 || whole.early == 0) fail("the files as given: a box failed, or no run was skipped or stopped early");
  for (size_t k = 0; k < 2; ++k)
    for (size_t len = 0; len < files[k].bytes.size(); ++len)
      if (len % (size_t)share == 0) run_one(files[k].bytes.data(), len, files[k].Hb, files[k].Wb, BOXES_DAMAGED, false, &cut);
  for (int k = 0; k < 6000; ++k) {
    const File& f = files[next() % files.size()];
    std::vector<uint8_t> b = f.bytes;
    // half of the mutations in the first 700 bytes (the marker segments), half anywhere (mostly the scan)
    const size_t at = (k & 1) ? next() % b.size() : next() % (b.size() < 700 ? b.size() : 700);
    b[at] = (k % 8 == 0) ? 0xFF : (uint8_t)next();
    if (k % share == 0) run_one(b.data(), b.size(), f.Hb, f.Wb, BOXES_DAMAGED, false, &mut);
  }
  report("as given:", whole);
  report("truncations:", cut);
  report("mutations:", mut);
  return 0;
}
