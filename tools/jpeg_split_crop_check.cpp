// Stand-alone host check of the device JPEG decode's SPLIT path FOR CROP BOXES on untrusted bytes (csrc/jpeg_split.h: seg_is_live,
// list_fits, write_walk<true>, zero_chroma_part_crop; csrc/jpeg_walk.h: check_box, crop_mcus, decode_run_crop -- the very text the lanes
// of rgbnm_jpeg_decode_batch_split_crop run, compiled here for the CPU).  The lanes are emulated one after another, pass by pass --
// map, scout, `rounds` sync rounds, verify with the live test and the compaction of the live slots into one list, the write pass over
// that list, then the one-lane crop walk for what is left -- and compared with what jpegwalk::decode_run alone gives on the same plan.
// Build it with the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/jpeg_split_crop_check.cpp -o jpeg_split_crop_check
//   ./jpeg_split_crop_check [--share D] DIR/*.jpg          (tools/jpeg_scan_files.py writes the test suite's files)
//
// Inputs (the driver of jpeg_check_common.h): every file as given, every truncation length of the first two, 6000 single-byte
// mutations from a fixed seed (--share D: every D-th truncation and mutation only).  Each goes through seg_bits 256 (runs of at least
// 16 segments are split) and 2048 (at least 2), each with rounds 0, 2 and 64, and through the largest even box and BOXES more from a
// fixed seed.  For every input that the parser accepts, every configuration and every box:
//   (a) the packed crops equal the box cut out of the plain walk's whole-grid output, every element of them written;
//   (b) status_whole <= status <= 0;   (c) status == 0 wherever status_whole == 0;   (d) path 1: status == status_whole;
//   seg_live equals a count that looks at every block of every segment, walked what the contract says per path; the guard bands
//   around both packed slots are untouched; the tile is zero after every walk; a segment that is not live is not in the list;
//   the compaction run with the runs in the opposite order (the list's order is the order of the runs' atomic adds) gives the same
//   packed crops, status, path, seg_live and walked, byte for byte.
// A bad box gives RGBNM_JPEG_EBOX with nothing written.  Heap blocks of the exact size throughout.  Exit status 0: clean.
#include "jpeg_check_common.h"
#include "../rgb-no-more_amd/csrc/jpeg_split.h"

using namespace jpegcheck;

static const int BOXES = 3, GUARD = 64;

struct Result {
  std::vector<int16_t> Yp, Cp;
  std::vector<uint32_t> walked, seg_live;
  int status = 0, path = 0;
  long segs = 0, live = 0;                                      // segments of the split runs that passed; of them, walked by the write pass
  bool operator==(const Result& o) const {
    return Yp == o.Yp && Cp == o.Cp && walked == o.walked && seg_live == o.seg_live && status == o.status && path == o.path;
  }
};

// does block b of the run lie in an MCU with a block inside its component's box?  By looking at every block of the MCU.
static bool brute_need(const rgbnm_jpeg_run& r, const rgbnm_jpeg_image& im, const int* box, uint64_t b) {
  const int m = r.mcu0 + (int)(b / (uint64_t)im.nblk), mx = m % im.mcus_x, my = m / im.mcus_x;
  for (int k = 0; k < im.nblk; ++k) {
    const int c = im.blk_comp[k], bx = mx * im.hs[c] + im.blk_dx[k], by = my * im.vs[c] + im.blk_dy[k];
    const int t = c ? box[0] / 2 : box[0], l = c ? box[1] / 2 : box[1], h = c ? box[2] / 2 : box[2], w = c ? box[3] / 2 : box[3];
    if (by >= t && by < t + h && bx >= l && bx < l + w) return true;
  }
  return false;
}
static uint32_t brute_walked(const rgbnm_jpeg_run& r, const rgbnm_jpeg_image& im, const int* box) {
  int last = -1;
  for (int m = 0; m < r.nmcu; ++m)
    if (brute_need(r, im, box, (uint64_t)m * (uint64_t)im.nblk)) last = m;
  return (uint32_t)(last + 1);
}

// One call.  reverse: verify (and with it the compaction) takes the runs last to first.  y_off / c_off: the slots' offsets.
static Result split_crop(const Plan& P, const int* box, long long y_off, long long c_off, int seg_bits, int min_seg, int rounds, bool reverse) {
  using namespace jpegsplit;
  const int Hb = P.Hb, Wb = P.Wb, Hbc = P.Hbc, Wbc = P.Wbc, nruns = P.p.nruns;
  const bool good = box[2] > 0 && box[3] > 0 && !((box[0] | box[1] | box[2] | box[3]) & 1) && box[2] <= Hb && box[3] <= Wb;
  const size_t ny = good ? (size_t)64 * box[2] * box[3] : 128, nc = good ? (size_t)128 * (box[2] / 2) * (box[3] / 2) : 128;
  Result R;
  R.Yp.assign((size_t)y_off + ny + GUARD, SENTINEL);
  R.Cp.assign((size_t)c_off + nc + GUARD, SENTINEL);
  R.walked.assign((size_t)nruns, 0xFFFFFFFFu);
  R.seg_live.assign((size_t)nruns, 0xFFFFFFFFu);
  const size_t bytes = crop_scratch_bytes(P.p.stream_bytes, nruns, seg_bits);
  if (!bytes || bytes < scratch_bytes(P.p.stream_bytes, nruns, seg_bits)) fail("crop_scratch_bytes refused the plan or is below the split bound");
  std::vector<uint64_t> mem((bytes + 7) / 8);                 // exact size (rounded to 8): the sanitizer sees any access past it
  Scratch s = carve(mem.data(), P.p.stream_bytes, nruns, seg_bits);
  Compact x = carve_crop(mem.data(), P.p.stream_bytes, nruns, seg_bits);
  if ((uint8_t*)(x.count + 1) > (uint8_t*)mem.data() + bytes) fail("the carved scratch is larger than its bound");
  const uint8_t* stream = P.stream.data();
  const rgbnm_jpeg_hufftab* tabs = P.tables.data();
  const jpegwalk::Out none = {0, 0, 0, 0, 0, nullptr, nullptr};
  alignas(16) int16_t tile[64] = {0};
  auto box_of = [&](jpegwalk::Crop* B) {
    return jpegwalk::check_box(box, y_off, c_off, Hb, Wb, Hbc, Wbc, R.Yp.data(), R.Yp.size() - GUARD, R.Cp.data(), R.Cp.size() - GUARD, B);
  };
  auto tile_zero = [&](const char* what) {
    for (int k = 0; k < 64; ++k)
      if (tile[k]) fail(what);
  };
  // init, map
  for (uint32_t i = 0; i < s.nslots; ++i) s.seg_run[i] = -1;
  *x.count = 0;
  std::vector<Lane> lanes((size_t)nruns);
  for (int ri = 0; ri < nruns; ++ri) {
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    RunInfo info = {0u, 0u};
    if (r.nmcu != 0) {
      if (jpegwalk::check_run(r, &P.image, 1, P.p.stream_bytes, P.p.ntables, &lanes[(size_t)ri]) != 0) fail("a run of the parser's fails check_run");
      info = map_run(r, ri, seg_bits, min_seg, s.nslots);
    }
    s.info[ri] = info;
    if (info.nseg && R.path < 1) R.path = 1;
    for (uint32_t j = 0; j < info.nseg; ++j) {
      if (s.seg_run[info.base + j] != -1) fail("two runs share a slot");
      s.seg_run[info.base + j] = ri;
    }
  }
  auto lane_of = [&](uint32_t slot, int* ri, uint32_t* j) {
    *ri = s.seg_run[slot];
    if (*ri < 0 || *ri >= nruns) return false;
    *j = slot - s.info[*ri].base;
    return *j < s.info[*ri].nseg;
  };
  // scout and the sync rounds: the split call's
  for (uint32_t slot = 0; slot < s.nslots; ++slot) {
    int ri;
    uint32_t j;
    if (!lane_of(slot, &ri, &j)) continue;
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    const uint64_t state = j == 0 ? pack_state(0, 0, 0) : seg_first_state(j, seg_bits);
    s.entry[slot] = state;
    s.exits[0][slot] = scout_walk(stream, r, lanes[(size_t)ri], tabs, state, seg_end(r, j, seg_bits), (uint32_t)seg_bits + 1u, &s.rec[slot]);
  }
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
    }
  }
  // verify, scan, live test and compaction, run by run in the given order
  const uint64_t* fin = s.exits[rounds & 1];
  for (int q = 0; q < nruns; ++q) {
    const int ri = reverse ? nruns - 1 - q : q;
    const RunInfo info = s.info[ri];
    x.live[ri] = RunLive{0u, 0u};
    if (!info.nseg) continue;
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    const Lane& L = lanes[(size_t)ri];
    jpegwalk::Crop B = {};
    const bool boxed = box_of(&B) == 0;
    const uint64_t N = (uint64_t)r.nmcu * (uint64_t)L.nblk;
    uint32_t carry[5] = {0, 0, 0, 0, 0}, nlive = 0;
    bool bad = false, found = false;
    for (uint32_t j = 0; j < info.nseg; ++j) {
      const uint32_t slot = info.base + j;
      const SegRec& c = s.rec[slot];
      if (s.seg_run[slot] != ri || s.entry[slot] != (j ? fin[slot - 1] : pack_state(0, 0, 0))) bad = true;
      const int verdict = seg_verdict(c, carry[0], N, r.nbytes * 8u);
      bad = bad || verdict == 1;
      found = found || verdict == 2;
      s.scan[slot].b0 = carry[1];
      for (int k = 0; k < 3; ++k) s.scan[slot].p[k] = carry[2 + k];
      if (boxed && seg_is_live(r, L, B, carry[1], c.nstart)) ++nlive;
      carry[0] += c.ndone;
      carry[1] += c.nstart;
      for (int k = 0; k < 3; ++k) carry[2 + k] += c.dc[k];
    }
    bool passed = !(bad || !found);
    uint32_t first = 0;
    if (passed && nlive) {
      first = *x.count;                                         // the atomic add
      *x.count += nlive;
      if (!list_fits(first, nlive, s.nslots)) fail("a run's live slots do not fit the list");
    }
    if (!passed) {
      nlive = 0;
      R.path = 2;
    }
    x.live[ri] = RunLive{first, nlive};
    uint32_t at = first;
    for (uint32_t j = 0; nlive && j < info.nseg; ++j) {
      const uint32_t slot = info.base + j;
      if (seg_is_live(r, L, B, s.scan[slot].b0, s.rec[slot].nstart)) {
        if (at - first >= nlive) fail("the second trip over a run finds more live segments than the first");
        x.list[at++] = slot;
      }
    }
    if (at - first != nlive) fail("the second trip over a run finds fewer live segments than the first");
  }
  // write, over the list
  const uint32_t nlist = *x.count < s.nslots ? *x.count : s.nslots;
  std::vector<char> listed(s.nslots, 0);
  for (uint32_t at = 0; at < nlist; ++at) {
    const uint32_t slot = x.list[at];
    int ri;
    uint32_t j;
    if (slot >= s.nslots || !lane_of(slot, &ri, &j)) fail("a list entry that is no segment's slot");
    if (listed[slot]++) fail("a slot is listed twice");
    if (R.path != 1) continue;
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    const Lane& L = lanes[(size_t)ri];
    jpegwalk::Crop B = {};
    if (box_of(&B) != 0) fail("a live segment behind a bad box");
    if (write_walk<true>(stream, r, L, tabs, jpegscan::ZIGZAG, none, tile, s.entry[slot], seg_end(r, j, seg_bits), (uint32_t)seg_bits + 64u,
                         s.scan[slot], B) != 0)
      fail("the write walk met what verify should have excluded");
    tile_zero("the tile is not zero after a segment");
    const RunLive rl = x.live[ri];
    if (at - rl.first >= rl.count) fail("a list entry outside its run's range");
    if (L.ncomp == 1) zero_chroma_part_crop(B, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total, at - rl.first, rl.count);
  }
  // what is left: decode_crop_rest_kernel's lane
  for (int ri = 0; ri < nruns; ++ri) {
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    uint32_t nwalk = 0, nlive = 0;
    jpegwalk::Crop B = {};
    const Lane& L = lanes[(size_t)ri];
    bool ok = r.nmcu != 0;
    if (ok && box_of(&B) != 0) {
      ok = false;
      if (RGBNM_JPEG_EBOX < R.status) R.status = RGBNM_JPEG_EBOX;
    } else if (ok && s.info[ri].nseg && R.path == 1) {
      nlive = x.live[ri].count;
      if (L.ncomp == 1 && nlive == 0) jpegwalk::zero_chroma_share_crop(B, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
      ok = false;
      R.segs += s.info[ri].nseg;
      R.live += nlive;
    } else if (ok) {
      nwalk = R.path == 1 ? (uint32_t)r.nmcu : jpegwalk::crop_mcus(r, L, B);
    }
    if (nwalk) {
      const int err = jpegwalk::decode_run_crop(stream, r, L, tabs, jpegscan::ZIGZAG, B, nwalk, tile);
      tile_zero("the tile is not zero after a crop run");
      if (err > 0) fail("a positive error code");
      if (err < R.status) R.status = err;
    }
    if (ok && L.ncomp == 1) jpegwalk::zero_chroma_share_crop(B, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
    R.walked[(size_t)ri] = nwalk;
    R.seg_live[(size_t)ri] = nlive;
  }
  // seg_live and walked against counts that look at every block, while the scratch is still here
  for (int ri = 0; good && ri < nruns; ++ri) {
    const rgbnm_jpeg_run& r = P.runs[(size_t)ri];
    if (r.nmcu == 0) continue;
    const RunInfo info = s.info[ri];
    uint32_t want_live = 0, want_walked = 0;
    if (info.nseg && R.path == 1) {
      const uint64_t N = (uint64_t)r.nmcu * (uint64_t)P.image.nblk;
      for (uint32_t j = 0; j < info.nseg; ++j) {
        const SegScan& sc = s.scan[info.base + j];
        uint64_t e = (uint64_t)sc.b0 + s.rec[info.base + j].nstart;
        e = e < N ? e : N;
        bool lv = false;
        for (uint64_t b = sc.b0; b < e; ++b) lv = lv || brute_need(r, P.image, box, b);
        want_live += lv ? 1u : 0u;
        if (!lv && listed[info.base + j]) fail("a segment that is not live is in the list");
      }
    } else {
      want_walked = R.path == 1 ? (uint32_t)r.nmcu : brute_walked(r, P.image, box);
    }
    if (R.seg_live[(size_t)ri] != want_live) fail("seg_live differs from the count over every block");
    if (R.walked[(size_t)ri] != want_walked) fail("walked differs from the count over every MCU");
  }
  return R;
}

struct Tally {
  long decoded = 0, refused_host = 0, refused_walk = 0, path[3] = {0, 0, 0};
  long calls = 0, clean = 0, hidden = 0, segs = 0, live = 0;
};

static void one_box(const Plan& P, const Grids& G, int status_whole, const int* box, Tally* t) {
  const int Wb = P.Wb, Hbc = P.Hbc, Wbc = P.Wbc;
  const size_t ny = (size_t)64 * box[2] * box[3], nc = (size_t)128 * (box[2] / 2) * (box[3] / 2);
  const long long y_off = GUARD + 8 * (long long)(next() % 5), c_off = GUARD + 8 * (long long)(next() % 5);
  const int cfg[2][2] = {{256, jpegsplit::MIN_SEG}, {2048, 2}};
  const int rounds[3] = {0, 2, 64};
  for (int c = 0; c < 2; ++c)
    for (int q = 0; q < 3; ++q) {
      const Result R = split_crop(P, box, y_off, c_off, cfg[c][0], cfg[c][1], rounds[q], false);
      if (!(R == split_crop(P, box, y_off, c_off, cfg[c][0], cfg[c][1], rounds[q], true)))
        fail("the outputs depend on the order of the runs in the list");
      for (size_t i = 0; i < R.Yp.size(); ++i)
        if ((i < (size_t)y_off || i >= (size_t)y_off + ny) && R.Yp[i] != SENTINEL) fail("a luma guard element changed");
      for (size_t i = 0; i < R.Cp.size(); ++i)
        if ((i < (size_t)c_off || i >= (size_t)c_off + nc) && R.Cp[i] != SENTINEL) fail("a chroma guard element changed");
      for (int y = 0; y < box[2]; ++y)
        for (int x = 0; x < box[3]; ++x)
          if (memcmp(&R.Yp[(size_t)y_off + ((size_t)y * box[3] + x) * 64], &G.Y[((size_t)(box[0] + y) * Wb + (box[1] + x)) * 64], 128))
            fail("a luma block of the crop differs from the whole-grid decode");
      const int hc = box[2] / 2, wc = box[3] / 2;
      for (int k = 0; k < 2; ++k)
        for (int y = 0; y < hc; ++y)
          for (int x = 0; x < wc; ++x)
            if (memcmp(&R.Cp[(size_t)c_off + (((size_t)k * hc + y) * wc + x) * 64],
                       &G.C[(((size_t)k * Hbc + (box[0] / 2 + y)) * Wbc + (box[1] / 2 + x)) * 64], 128))
              fail("a chroma block of the crop differs from the whole-grid decode");
      if (!(status_whole <= R.status && R.status <= 0)) fail("status_whole <= status <= 0 does not hold");
      if (status_whole == 0 && R.status != 0) fail("the call fails a file the whole decode accepts");
      if (R.path == 1 && R.status != status_whole) fail("path 1 with a status that is not the whole decode's");
      if (R.path < 0 || R.path > 2) fail("path out of range");
      ++t->path[R.path];
      ++t->calls;
      if (R.status == 0) ++t->clean;
      if (R.status == 0 && status_whole != 0) ++t->hidden;
      t->segs += R.segs;
      t->live += R.live;
    }
}

// a bad box: RGBNM_JPEG_EBOX, nothing written, nothing walked
static void bad_box(const Plan& P) {
  const int boxes[3][4] = {{1, 0, 2, 2}, {0, 0, (P.Hb & ~1) + 2, 2}, {0, 2, 2, 0}};
  for (const int* box : {boxes[0], boxes[1], boxes[2]}) {
    const Result R = split_crop(P, box, GUARD, GUARD, 2048, 2, 64, false);
    if (R.status != RGBNM_JPEG_EBOX) fail("a bad box was not refused");
    for (int16_t v : R.Yp)
      if (v != SENTINEL) fail("a bad box, and luma was written");
    for (int16_t v : R.Cp)
      if (v != SENTINEL) fail("a bad box, and chroma was written");
    for (size_t i = 0; i < R.walked.size(); ++i)
      if (R.walked[i] || R.seg_live[i]) fail("a bad box, and a run was walked");
  }
}

static int run_one(const uint8_t* bytes, size_t len, int Hb, int Wb, bool given, Tally* t) {
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
  if (given) {
    bad_box(P);
    const int box[4] = {0, 0, he, we};
    one_box(P, G, status, box, t);
  }
  for (int k = 0; k < (given ? BOXES : 1); ++k) {
    int box[4];
    box[2] = 2 * (1 + (int)(next() % (uint64_t)(he / 2)));
    box[3] = 2 * (1 + (int)(next() % (uint64_t)(we / 2)));
    if (k % 2 == 0) box[2] = box[2] > 4 ? 2 : box[2], box[3] = box[3] > 4 ? 2 : box[3];     // small boxes skip the most
    box[0] = 2 * (int)(next() % (uint64_t)((he - box[2]) / 2 + 1));
    box[1] = 2 * (int)(next() % (uint64_t)((we - box[3]) / 2 + 1));
    one_box(P, G, status, box, t);
  }
  return status;
}

int main(int argc, char** argv) {
  Tally tally[3];                                               // as given, truncations, mutations
  const int rc = drive(argc, argv, "jpeg_split_crop_check", [&](Kind kind, const File& f, const uint8_t* bytes, size_t len) {
    return run_one(bytes, len, f.Hb, f.Wb, kind == AS_GIVEN, &tally[kind]);
  });
  if (rc) return rc;
  const Tally& g = tally[AS_GIVEN];
  if (g.refused_walk) fail("a file as given got as far as the walk and was refused there");
  if (g.clean != g.calls || g.path[1] == 0 || g.live == 0 || g.live == g.segs) fail("the files as given: a call failed, none was split, or no segment was live or skipped");
  const char* names[3] = {"as given:   ", "truncations:", "mutations:  "};
  for (int i = 0; i < 3; ++i)
    printf("%s %ld decoded, %ld refused by the parser, %ld by the walk; %ld calls: %ld clean (%ld of them hide a later error), %ld not split, "
           "%ld split, %ld split then one-lane; %ld of %ld segments live\n",
           names[i], tally[i].decoded, tally[i].refused_host, tally[i].refused_walk, tally[i].calls, tally[i].clean, tally[i].hidden,
           tally[i].path[0], tally[i].path[1], tally[i].path[2], tally[i].live, tally[i].segs);
  return 0;
}
