// Host half of the device JPEG entropy decode (include/rgbnm.h, rgbnm_jpeg_prepare): find the independent bit streams of baseline
// JPEG files.  Plain C++, no HIP: tools/jpeg_scan_check.cpp includes it and runs it under the host sanitizers.
//
// Two passes.  The header pass (serial, cheap) parses the marker segments of every file up to its scan, checks what the device
// walk can decode, de-duplicates the Huffman tables of the batch and lays out each file's region of the stream and its run records
// -- their number is known from the header: ceil(MCUs / restart interval).  The scan pass (files are independent, so a few
// threads may share them) copies the entropy-coded bytes into the region, dropping the stuffed zero behind every FF and splitting
// at the RSTn markers, and fills the records.  The bytes are untrusted: every length is checked against the file before use.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../../include/rgbnm.h"

namespace jpegscan {

// zig-zag position -> natural (row-major) position in the 8 x 8 block (ITU-T T.81 figure A.6)
#define JPEGSCAN_ZIGZAG_VALUES                                                                                                      \
  0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, \
      57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63
static const uint8_t ZIGZAG[64] = {JPEGSCAN_ZIGZAG_VALUES};

// a file between the two passes
struct Pending {
  size_t scan_pos = 0;        // first entropy-coded byte
  size_t region = 0, region_cap = 0;
  int run0 = 0, nruns = 0;
  int restart = 0, nmcu = 0;
};

struct RawTable {
  bool set = false;
  uint8_t bits[16], vals[256];
  int nvals = 0;
};

static inline int fail(rgbnm_jpeg_plan* p, int i, int code, const char* msg) {
  p->images[i].status = code;
  if (p->messages && p->message_len > 0) snprintf(p->messages + (size_t)i * p->message_len, (size_t)p->message_len, "%s", msg);
  return code;
}

// libjpeg's jpeg_make_d_derived_tbl: canonical codes, with its consistency checks.  false: the counts do not form a prefix code.
static inline bool derive(const RawTable& r, rgbnm_jpeg_hufftab* t) {
  memset(t, 0, sizeof(*t));
  memcpy(t->bits, r.bits, 16);
  memcpy(t->vals, r.vals, (size_t)r.nvals);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = r.bits[l - 1];
    if (cnt) {
      if (code + cnt > (1 << l)) return false;  // more codes of this length than the prefix leaves room for: before `look` is indexed
      t->valoff[l] = k - code;
      for (int j = 0; j < cnt; ++j, ++k, ++code)
        if (l <= 9) {
          const int lo = code << (9 - l);
          for (int f = 0; f < (1 << (9 - l)); ++f) t->look[lo + f] = (uint16_t)((l << 8) | r.vals[k]);
        }
      t->maxcode[l] = code - 1;
    } else {
      t->maxcode[l] = -1;
    }
    code <<= 1;
  }
  t->maxcode[0] = -1;
  t->maxcode[17] = 0xFFFFF;
  return true;
}

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Header pass of file i.  Returns 0 with *pd filled (stream region and run records reserved in *stream_used / *runs_used), or the
// negative status it stored.
static inline int parse_header(const uint8_t* d, size_t n, int i, int Hb, int Wb, int Hbc, int Wbc, rgbnm_jpeg_plan* p, Pending* pd,
                               size_t* stream_used, int* runs_used) {
  rgbnm_jpeg_image* im = &p->images[i];
  memset(im, 0, sizeof(*im));
  int16_t* q = p->quant + (size_t)i * 192;
  for (int k = 0; k < 192; ++k) q[k] = 1;
  if (p->messages && p->message_len > 0) p->messages[(size_t)i * p->message_len] = 0;
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(p, i, n < 4 ? RGBNM_JPEG_ETRUNCATED : RGBNM_JPEG_EMARKER, "no SOI marker");
  uint16_t qt[4][64];
  bool qset[4] = {false, false, false, false};
  RawTable ht[2][4];
  bool sof = false;
  int ncomp = 0, width = 0, height = 0, restart = 0;
  int cid[3] = {0, 0, 0}, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1}, tq[3] = {0, 0, 0};
  size_t pos = 2;
  for (;;) {
    // next marker: FF, any number of fill FFs, the code
    if (pos >= n) return fail(p, i, RGBNM_JPEG_ETRUNCATED, "file ends before the scan");
    if (d[pos] != 0xFF) return fail(p, i, RGBNM_JPEG_EMARKER, "marker expected");
    while (pos < n && d[pos] == 0xFF) ++pos;
    if (pos >= n) return fail(p, i, RGBNM_JPEG_ETRUNCATED, "file ends inside a marker");
    const int m = d[pos++];
    if (m == 0x01 || m == 0xD8) continue;                       // TEM, a second SOI: no segment
    if (m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return fail(p, i, RGBNM_JPEG_EMARKER, "restart marker or stuffed byte outside a scan");
    if (m == 0xD9) return fail(p, i, RGBNM_JPEG_EMARKER, "EOI before a scan");
    if (pos + 2 > n) return fail(p, i, RGBNM_JPEG_ETRUNCATED, "file ends inside a segment length");
    const int len = be16(d + pos);
    if (len < 2) return fail(p, i, RGBNM_JPEG_EMARKER, "segment length below 2");
    if (pos + (size_t)len > n) return fail(p, i, RGBNM_JPEG_ETRUNCATED, "segment runs past the end of the file");
    const uint8_t* s = d + pos + 2;
    const int sl = len - 2;
    pos += (size_t)len;
    if (m == 0xDB) {                                            // DQT: one or more tables, zig-zag order in the file
      int o = 0;
      while (o < sl) {
        const int pq = s[o] >> 4, t = s[o] & 15;
        if (pq > 1 || t > 3 || o + 1 + 64 * (pq + 1) > sl) return fail(p, i, RGBNM_JPEG_EMARKER, "bad DQT segment");
        for (int k = 0; k < 64; ++k) qt[t][ZIGZAG[k]] = pq ? (uint16_t)be16(s + o + 1 + 2 * k) : s[o + 1 + k];
        qset[t] = true;
        o += 1 + 64 * (pq + 1);
      }
    } else if (m == 0xC4) {                                     // DHT: one or more tables
      int o = 0;
      while (o < sl) {
        if (o + 17 > sl) return fail(p, i, RGBNM_JPEG_EMARKER, "bad DHT segment");
        const int tc = s[o] >> 4, t = s[o] & 15;
        int cnt = 0;
        for (int k = 0; k < 16; ++k) cnt += s[o + 1 + k];
        if (tc > 1 || t > 3 || cnt > 256 || o + 17 + cnt > sl) return fail(p, i, RGBNM_JPEG_EMARKER, "bad DHT segment");
        RawTable& r = ht[tc][t];
        r.set = true;
        r.nvals = cnt;
        memcpy(r.bits, s + o + 1, 16);
        memset(r.vals, 0, 256);
        memcpy(r.vals, s + o + 17, (size_t)cnt);
        o += 17 + cnt;
      }
    } else if (m == 0xDD) {                                     // DRI
      if (sl != 2) return fail(p, i, RGBNM_JPEG_EMARKER, "bad DRI segment");
      restart = be16(s);
    } else if (m == 0xC0 || m == 0xC1) {                        // SOF0 / SOF1
      if (sof) return fail(p, i, RGBNM_JPEG_EMARKER, "second frame header");
      if (sl < 6) return fail(p, i, RGBNM_JPEG_EMARKER, "bad SOF segment");
      if (s[0] != 8) return fail(p, i, RGBNM_JPEG_EUNSUPPORTED, "sample precision is not 8 bits");
      height = be16(s + 1);
      width = be16(s + 3);
      ncomp = s[5];
      if (height == 0) return fail(p, i, RGBNM_JPEG_EUNSUPPORTED, "height comes in a DNL marker");
      if (width == 0) return fail(p, i, RGBNM_JPEG_EMARKER, "zero width");
      if (ncomp != 1 && ncomp != 3) return fail(p, i, RGBNM_JPEG_EUNSUPPORTED, "1 or 3 components are decoded on the device");
      if (sl != 6 + 3 * ncomp) return fail(p, i, RGBNM_JPEG_EMARKER, "bad SOF segment");
      for (int c = 0; c < ncomp; ++c) {
        cid[c] = s[6 + 3 * c];
        hs[c] = s[7 + 3 * c] >> 4;
        vs[c] = s[7 + 3 * c] & 15;
        tq[c] = s[8 + 3 * c];
        if (hs[c] < 1 || hs[c] > 4 || vs[c] < 1 || vs[c] > 4 || tq[c] > 3) return fail(p, i, RGBNM_JPEG_EMARKER, "bad SOF component");
      }
      sof = true;
    } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC8) {         // every other frame type, DAC (arithmetic conditioning)
      return fail(p, i, RGBNM_JPEG_EUNSUPPORTED,
                  m == 0xC2 ? "progressive file" : (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) ? "lossless file"
                                                 : m >= 0xC9 ? "arithmetic coding" : "differential frame");
    } else if (m == 0xDC) {
      return fail(p, i, RGBNM_JPEG_EUNSUPPORTED, "DNL marker");
    } else if (m == 0xDA) {                                     // SOS: the one scan
      if (!sof) return fail(p, i, RGBNM_JPEG_EMARKER, "scan before the frame header");
      if (sl < 1) return fail(p, i, RGBNM_JPEG_EMARKER, "bad SOS segment");
      const int ns = s[0];
      if (ns < 1 || ns > 4 || sl != 4 + 2 * ns) return fail(p, i, RGBNM_JPEG_EMARKER, "bad SOS segment");
      if (ns != ncomp) return fail(p, i, RGBNM_JPEG_EUNSUPPORTED, "several scans (one interleaved scan is decoded on the device)");
      int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != cid[c]) return fail(p, i, RGBNM_JPEG_EUNSUPPORTED, "scan components not in frame order");
        td[c] = s[2 + 2 * c] >> 4;
        ta[c] = s[2 + 2 * c] & 15;
        if (td[c] > 3 || ta[c] > 3 || !ht[0][td[c]].set || !ht[1][ta[c]].set) return fail(p, i, RGBNM_JPEG_EMARKER, "scan names an undefined Huffman table");
        if (!qset[tq[c]]) return fail(p, i, RGBNM_JPEG_EMARKER, "component names an undefined quantisation table");
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return fail(p, i, RGBNM_JPEG_EUNSUPPORTED, "spectral selection or successive approximation");
      // geometry (T.81 A.1.1, A.2): the grids of the components and the MCU layout
      int hmax = 1, vmax = 1;
      for (int c = 0; c < ncomp; ++c) {
        hmax = hs[c] > hmax ? hs[c] : hmax;
        vmax = vs[c] > vmax ? vs[c] : vmax;
      }
      int gw[3], gh[3];
      for (int c = 0; c < ncomp; ++c) {
        gw[c] = ((width * hs[c] + hmax - 1) / hmax + 7) / 8;
        gh[c] = ((height * vs[c] + vmax - 1) / vmax + 7) / 8;
      }
      if (gh[0] != Hb || gw[0] != Wb || (ncomp == 3 && (gh[1] != Hbc || gw[1] != Wbc || gh[2] != Hbc || gw[2] != Wbc)))
        return fail(p, i, RGBNM_JPEG_EGRID, "coefficient grid differs from the batch shape");
      im->ncomp = ncomp;
      if (ncomp == 1) {                                         // a one-component scan is not interleaved: one block per MCU
        im->mcus_x = gw[0];
        im->mcus_y = gh[0];
        im->nblk = 1;
        im->hs[0] = im->vs[0] = 1;
      } else {
        im->mcus_x = (width + 8 * hmax - 1) / (8 * hmax);
        im->mcus_y = (height + 8 * vmax - 1) / (8 * vmax);
        int b = 0;
        for (int c = 0; c < 3; ++c) {
          im->hs[c] = hs[c];
          im->vs[c] = vs[c];
          if (b + hs[c] * vs[c] > 10) return fail(p, i, RGBNM_JPEG_EUNSUPPORTED, "more than 10 blocks per MCU");
          for (int y = 0; y < vs[c]; ++y)
            for (int x = 0; x < hs[c]; ++x, ++b) {
              im->blk_comp[b] = c;
              im->blk_dx[b] = x;
              im->blk_dy[b] = y;
            }
        }
        im->nblk = b;
      }
      for (int c = 0; c < ncomp; ++c)
        for (int k = 0; k < 64; ++k) q[c * 64 + k] = (int16_t)qt[tq[c]][k];
      // tables: every distinct (bits, vals) once per batch
      for (int c = 0; c < ncomp; ++c)
        for (int ac = 0; ac < 2; ++ac) {
          const RawTable& r = ht[ac][ac ? ta[c] : td[c]];
          int found = -1;
          for (int t = 0; t < p->ntables && found < 0; ++t)
            if (!memcmp(p->tables[t].bits, r.bits, 16) && !memcmp(p->tables[t].vals, r.vals, 256)) found = t;
          if (found < 0) {
            if (p->ntables >= p->tables_cap || p->ntables >= 65535) return fail(p, i, RGBNM_JPEG_ECAPACITY, "table buffer of the plan is full");
            if (!derive(r, &p->tables[p->ntables])) return fail(p, i, RGBNM_JPEG_EMARKER, "Huffman table is not a prefix code");
            found = p->ntables++;
          }
          (ac ? im->ac_tab : im->dc_tab)[c] = found;
        }
      const long long nmcu = (long long)im->mcus_x * im->mcus_y;
      const long long nruns = restart ? (nmcu + restart - 1) / restart : 1;
      const size_t scan_len = n - pos;
      const size_t cap = ((scan_len + 3) & ~(size_t)3) + 8 * (size_t)nruns;
      if (nruns > p->runs_cap - *runs_used || cap > p->stream_cap - *stream_used) return fail(p, i, RGBNM_JPEG_ECAPACITY, "stream or run buffer of the plan is too small");
      pd->scan_pos = pos;
      pd->region = *stream_used;
      pd->region_cap = cap;
      pd->run0 = *runs_used;
      pd->nruns = (int)nruns;
      pd->restart = restart;
      pd->nmcu = (int)nmcu;
      im->nruns = (int)nruns;
      for (int r = 0; r < (int)nruns; ++r) {
        rgbnm_jpeg_run* rr = &p->runs[pd->run0 + r];
        memset(rr, 0, sizeof(*rr));
        rr->image = i;
      }
      *stream_used += cap;
      *runs_used += (int)nruns;
      return 0;
    }
    // APPn, COM and everything else with a length: skipped
  }
}

// Scan pass of file i: un-stuff into the file's region, one record per run.  Returns 0 or the negative status it stored (the file's
// records then stay empty, nmcu == 0, and the device skips them).
static inline int scan_file(const uint8_t* d, size_t n, int i, rgbnm_jpeg_plan* p, const Pending& pd) {
  uint8_t* out = p->stream + pd.region;
  const size_t cap = pd.region_cap;
  size_t o = 0, run_start = 0, pos = pd.scan_pos;
  int run = 0, code = 0;
  const char* why = nullptr;
  std::vector<rgbnm_jpeg_run> recs((size_t)pd.nruns);
  // closes the run [run_start, o): record, zero padding to the next multiple of 4 and 4 more
  auto close = [&]() -> bool {
    if (run >= pd.nruns) return false;
    rgbnm_jpeg_run& r = recs[(size_t)run];
    memset(&r, 0, sizeof(r));
    r.offset = (uint32_t)(pd.region + run_start);
    r.nbytes = (uint32_t)(o - run_start);
    r.image = i;
    r.mcu0 = pd.restart ? run * pd.restart : 0;
    r.nmcu = pd.restart && (run + 1) * (long long)pd.restart < pd.nmcu ? pd.restart : pd.nmcu - r.mcu0;
    const size_t end = ((o + 3) & ~(size_t)3) + 4;
    if (end > cap) return false;
    memset(out + o, 0, end - o);
    o = run_start = end;
    ++run;
    return true;
  };
  for (;;) {
    const uint8_t* f = pos < n ? (const uint8_t*)memchr(d + pos, 0xFF, n - pos) : nullptr;
    if (!f) { code = RGBNM_JPEG_ETRUNCATED; why = "file ends inside the scan"; break; }
    const size_t take = (size_t)(f - (d + pos));
    if (o + take + 1 > cap) { code = RGBNM_JPEG_ECAPACITY; why = "scan larger than its region"; break; }
    memcpy(out + o, d + pos, take);
    o += take;
    pos += take + 1;                                            // behind the FF
    while (pos < n && d[pos] == 0xFF) ++pos;                    // fill bytes
    if (pos >= n) { code = RGBNM_JPEG_ETRUNCATED; why = "file ends inside the scan"; break; }
    const int m = d[pos++];
    if (m == 0) { out[o++] = 0xFF; continue; }                  // a stuffed FF 00: the data byte FF
    if (m >= 0xD0 && m <= 0xD7) {
      if (!pd.restart || m != 0xD0 + (run & 7)) { code = RGBNM_JPEG_ERESTART; why = "restart marker out of sequence"; break; }
      if (!close()) { code = RGBNM_JPEG_ERESTART; why = "more runs than ceil(MCUs / restart interval)"; break; }
      continue;
    }
    // any other marker ends the scan
    if (!close() || run != pd.nruns) { code = RGBNM_JPEG_ERESTART; why = "run count is not ceil(MCUs / restart interval)"; break; }
    if (m == 0xD9) break;                                       // EOI
    if (m == 0xDC) { code = RGBNM_JPEG_EUNSUPPORTED; why = "DNL marker"; break; }
    if (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD) { code = RGBNM_JPEG_EUNSUPPORTED; why = "several scans"; break; }
    code = RGBNM_JPEG_EMARKER; why = "unexpected marker behind the scan";
    break;
  }
  if (code) return fail(p, i, code, why);
  memcpy(p->runs + pd.run0, recs.data(), recs.size() * sizeof(rgbnm_jpeg_run));
  return 0;
}

static inline int prepare(const uint8_t* const* bufs, const size_t* lens, int n, int Hb, int Wb, int Hbc, int Wbc, rgbnm_jpeg_plan* p) {
  if (!bufs || !lens || !p || n <= 0 || Hb < 1 || Wb < 1 || Hbc < 1 || Wbc < 1 || Hb > 4096 || Wb > 4096 || Hbc > 4096 || Wbc > 4096)
    return -1;                                                  // RGBNM_EINVAL
  if (!p->stream || !p->runs || !p->images || !p->tables || !p->quant || p->runs_cap <= 0 || p->tables_cap <= 0 || p->stream_cap == 0 ||
      p->stream_cap > 0xFFFFFFF0u)
    return -1;                                                  // RGBNM_EINVAL
  p->ntables = 0;
  size_t stream_used = 0;
  int runs_used = 0;
  std::vector<Pending> pend((size_t)n);
  for (int i = 0; i < n; ++i) parse_header(bufs[i], lens[i], i, Hb, Wb, Hbc, Wbc, p, &pend[(size_t)i], &stream_used, &runs_used);
  int threads = p->threads < 1 ? 1 : p->threads > 16 ? 16 : p->threads;
  if (threads > n) threads = n;
  auto work = [&](int t) {
    for (int i = t; i < n; i += threads)
      if (p->images[i].status == 0) scan_file(bufs[i], lens[i], i, p, pend[(size_t)i]);
  };
  if (threads == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (int t = 1; t < threads; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
  }
  p->stream_bytes = stream_used;
  p->nruns = runs_used;
  p->nbad = 0;
  for (int i = 0; i < n; ++i) p->nbad += p->images[i].status != 0;
  return p->nbad;
}

}  // namespace jpegscan
