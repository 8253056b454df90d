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
#include "jpeg_check_common.h"

using namespace jpegcheck;

static const int BOXES_GIVEN = 12, BOXES_DAMAGED = 2, GUARD = 64;

struct Tally {
  long decoded = 0, refused_host = 0, refused_walk = 0;        // inputs, by the plain walk's verdict
  long boxes = 0, crop_clean = 0;                              // boxes tried; of them, status_crop == 0
  long hidden = 0;                                             // ... while status_whole < 0: the error lay behind the last needed MCU
  long runs = 0, skipped = 0, early = 0;                       // runs seen by a box; not walked; stopped before their end
  long long mcus = 0, walked = 0;
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
  Plan P;
  if (const int st = prepare(P, bytes, len, Hb, Wb)) {
    ++t->refused_host;
    return st;
  }
  Grids G(P);
  const int status = plain_walk(P, G);
  if (status) ++t->refused_walk; else ++t->decoded;
  const int he = Hb & ~1, we = Wb & ~1;
  if (he < 2 || we < 2) return status;                          // no even box fits this grid
  if (largest) {
    const int box[4] = {0, 0, he, we};
    one_box(P, Hb, Wb, box, G.Y, G.C, status, t);
  }
  for (int k = 0; k < nbox; ++k) {
    int box[4];
    box[2] = 2 * (1 + (int)(next() % (uint64_t)(he / 2)));
    box[3] = 2 * (1 + (int)(next() % (uint64_t)(we / 2)));
    if (k % 3 == 0) box[2] = box[2] > 4 ? 2 : box[2], box[3] = box[3] > 4 ? 2 : box[3];     // small boxes skip the most
    box[0] = 2 * (int)(next() % (uint64_t)((he - box[2]) / 2 + 1));
    box[1] = 2 * (int)(next() % (uint64_t)((we - box[3]) / 2 + 1));
    one_box(P, Hb, Wb, box, G.Y, G.C, status, t);
  }
  return status;
}

static void report(const char* what, const Tally& t) {
  printf("%-12s %ld decoded, %ld refused by the parser, %ld by the walk; %ld boxes: %ld clean (%ld of them hide a later error), "
         "%ld runs: %ld skipped, %ld stopped early, %lld of %lld MCUs walked\n",
         what, t.decoded, t.refused_host, t.refused_walk, t.boxes, t.crop_clean, t.hidden, t.runs, t.skipped, t.early, t.walked, t.mcus);
}

int main(int argc, char** argv) {
  Tally tally[3];                                               // as given, truncations, mutations
  const int rc = drive(argc, argv, "jpeg_crop_check", [&](Kind kind, const File& f, const uint8_t* bytes, size_t len) {
    if (kind == AS_GIVEN) bad_boxes(f.Hb, f.Wb);
    return run_one(bytes, len, f.Hb, f.Wb, kind == AS_GIVEN ? BOXES_GIVEN : BOXES_DAMAGED, kind == AS_GIVEN, &tally[kind]);
  });
  if (rc) return rc;
  const Tally& whole = tally[AS_GIVEN];
  if (whole.crop_clean != whole.boxes || whole.skipped == 0 || whole.early == 0) fail("the files as given: a box failed, or no run was skipped or stopped early");
  report("as given:", whole);
  report("truncations:", tally[TRUNCATION]);
  report("mutations:", tally[MUTATION]);
  return 0;
}
