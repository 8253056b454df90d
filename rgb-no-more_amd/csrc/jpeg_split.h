// The split decode of the device JPEG path (include/rgbnm.h, rgbnm_jpeg_decode_batch_split): a run is cut into bit segments of
// seg_bits, ONE LANE PER SEGMENT, and the lanes find the true parse by the self-synchronisation of Huffman codes (Klein & Wiseman;
// Weissenberger & Schmidt).  Like jpeg_walk.h this is __host__ __device__ text over plain pointers: jpeg_decode.hip runs it per lane,
// tools/jpeg_split_check.cpp runs the same text on the CPU under the host sanitizers, lane after lane, pass by pass.
//
// The passes (each a launch; a lane touches its own segment's records only and reads its predecessor's from the launch before;
// the one word a launch both reads and writes is path[image] in the write pass, raised to 2 by a lane whose walk failed -- harmless,
// the one-lane walk behind it rewrites that image whatever the other lanes saw):
//   map     per run: number of segments, first slot, split or not.  Slot of segment j of run i: floor(offset * 8 / seg_bits) + i + j;
//           the runs lie in the stream in record order without overlap, so the slot ranges do not overlap either (a run's segments
//           number at most floor(distance to the next run * 8 / seg_bits) + 1) and no scan is needed to place them.  That order is
//           rgbnm_jpeg_prepare's and a precondition of the call; runs that break it stay memory-safe (every lane re-checks its slot,
//           run and image) and verify fails a run one of whose slots another run took, so it goes to the one-lane walk.
//   scout   segment 0 starts in the true state (bit 0, k = 0, blk = 0), every other at its first bit with (k = 0, blk = 0).  The lane
//           walks symbols until it is at or past the segment's end and records the exit state and what it met (SegRec).
//   sync    `rounds` times: a segment whose entry differs from its predecessor's exit OF THE ROUND BEFORE (the exits are double
//           buffered, so a round is a Jacobi step whatever the order of the lanes) walks again from that exit.  After round j the
//           segments 0..j are true, so a run of at most rounds + 1 segments is certain to converge.
//   verify  per run: converged (every entry equals the predecessor's exit); the block that completes as number nmcu * nblk is the
//           last to complete in its segment, at a position that leaves at most 8 bits; no walk met an impossible symbol up to there.
//           An exclusive scan gives each segment the index of the first block that starts in it and the DC predictors there.
//   write   per segment of a run that passed: skip the block under way at the entry, decode every block whose DC symbol starts
//           before the segment's end -- on past the end until the last of them is complete -- and store through flush_block.
// Every image with a run that did not pass is decoded by the one-lane walk afterwards, as are the runs that were not split.
// The crop form (rgbnm_jpeg_decode_batch_split_crop; the last part of this file): the same passes up to verify, then the write pass
// over a compacted list of the segments that hold a block of the image's crop box, into the packed crop.
//
// Safety (the bytes are untrusted): a walk that meets an impossible symbol carries on -- it skips one bit of an unassigned code,
// clamps a coefficient index past 63, ignores the run nibble of a DC symbol -- and notes it, because a walk from a guessed state
// meets such symbols in well-formed streams and would otherwise never fall into step.  Every trip consumes at least one bit; trips
// are bounded by seg_bits + 1 (scout, sync) or seg_bits + 64 (write); reads of the stream are clamped to the run's words; stores go
// through flush_block's range check.  The write walk stops at the first impossible symbol and reports it (that cannot happen after
// verify; the image then goes to the one-lane walk like any that failed).  Nothing waits for another lane.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jpeg_walk.h"

namespace jpegsplit {

using jpegwalk::Bits;                                      // the symbol reader is jpeg_walk.h's
using jpegwalk::bits_open;
using jpegwalk::Lane;
using jpegwalk::next_symbol;
using jpegwalk::Out;
using jpegwalk::Sym;
using jpegwalk::table_of;

constexpr int SEG_BITS_MIN = 128, SEG_BITS_MAX = 65536;    // a multiple of 32 in this range
constexpr int ROUNDS_MAX = 64;
constexpr int MIN_SEG = 16;                                // runs of fewer segments are not split (option "jpeg_min_seg")
constexpr uint32_t ERR_ANY = 1u, ERR_DONE = 2u;            // SegRec.err: an impossible symbol anywhere / up to the last completed block

// a parse state in one word, so that it is loaded, stored and compared whole: bit position in the run | k << 32 | blk << 40
__host__ __device__ inline uint64_t pack_state(uint32_t pos, int k, int blk) { return (uint64_t)pos | ((uint64_t)k << 32) | ((uint64_t)blk << 40); }
__host__ __device__ inline uint32_t state_pos(uint64_t s) { return (uint32_t)s; }
__host__ __device__ inline int state_k(uint64_t s) { return (int)(s >> 32) & 63; }
__host__ __device__ inline int state_blk(uint64_t s) { return (int)(s >> 40) & 15; }

struct RunInfo { uint32_t base, nseg; };                   // first slot; segments, 0: the run is not split
// what a scout / sync walk met: DC symbols decoded (= blocks that start in the segment), blocks completed, the position behind the
// last completed block, the sums of the DC differences per component (wrapping, like the int sums of decode_run)
struct SegRec { uint32_t nstart, ndone, done_pos, err, dc[3], _pad; };   // 32 bytes
struct SegScan { uint32_t b0, p[3]; };                     // first block that starts in the segment; predictors at its entry

struct Scratch {
  RunInfo* info;        // [nruns]
  int32_t* seg_run;     // [nslots]: run of the slot, -1: none
  uint64_t* entry;      // [nslots]
  uint64_t* exits[2];   // [nslots] each: the exits of the round before / of this round
  SegRec* rec;          // [nslots]
  SegScan* scan;        // [nslots]
  uint32_t nslots;
};

inline size_t slot_count(size_t stream_bytes, int nruns, int seg_bits) { return stream_bytes * 8 / (size_t)seg_bits + (size_t)nruns + 1; }
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
// 0: arguments out of range (or more slots than 32 bits index)
inline size_t scratch_bytes(size_t stream_bytes, int nruns, int seg_bits) {
  if (nruns < 0 || seg_bits < SEG_BITS_MIN || seg_bits > SEG_BITS_MAX || (seg_bits & 31) || stream_bytes > ((size_t)1 << 40)) return 0;
  const size_t S = slot_count(stream_bytes, nruns, seg_bits);
  if (S > 0x7FFFFFFFu) return 0;
  return align16((size_t)nruns * sizeof(RunInfo)) + align16(S * 4) + 3 * align16(S * 8) + S * sizeof(SegRec) + S * sizeof(SegScan);
}
inline Scratch carve(void* mem, size_t stream_bytes, int nruns, int seg_bits) {
  const size_t S = slot_count(stream_bytes, nruns, seg_bits);
  uint8_t* p = static_cast<uint8_t*>(mem);
  Scratch s;
  s.info = reinterpret_cast<RunInfo*>(p); p += align16((size_t)nruns * sizeof(RunInfo));
  s.seg_run = reinterpret_cast<int32_t*>(p); p += align16(S * 4);
  s.entry = reinterpret_cast<uint64_t*>(p); p += align16(S * 8);
  s.exits[0] = reinterpret_cast<uint64_t*>(p); p += align16(S * 8);
  s.exits[1] = reinterpret_cast<uint64_t*>(p); p += align16(S * 8);
  s.rec = reinterpret_cast<SegRec*>(p); p += S * sizeof(SegRec);
  s.scan = reinterpret_cast<SegScan*>(p);
  s.nslots = (uint32_t)S;
  return s;
}

// map: segments and first slot of run `ri` (its record has passed check_run).  nseg = 0: not split.
__host__ __device__ inline RunInfo map_run(const rgbnm_jpeg_run& r, int ri, int seg_bits, int min_seg, uint32_t nslots) {
  const uint64_t bits = (uint64_t)r.nbytes * 8u, sb = (uint64_t)seg_bits;
  const uint64_t nseg = (bits + sb - 1) / sb, base = (uint64_t)r.offset * 8u / sb + (uint64_t)ri;
  RunInfo i = {(uint32_t)(base < nslots ? base : 0), 0u};
  if (nseg >= (uint64_t)(min_seg < 2 ? 2 : min_seg) && base + nseg <= (uint64_t)nslots) i.nseg = (uint32_t)nseg;
  return i;
}

// scout / sync: walk from `state` until at or past `end` (a bit position of the run, <= its bit count); stores nothing.  Returns the
// exit state and fills *rec.
__host__ __device__ inline uint64_t scout_walk(const uint8_t* stream, const rgbnm_jpeg_run& r, const Lane& L, const rgbnm_jpeg_hufftab* tabs,
                                               uint64_t state, uint32_t end, uint32_t maxtrips, SegRec* rec) {
  uint32_t pos = state_pos(state);
  int k = state_k(state), blk = state_blk(state);
  if (blk >= L.nblk) blk = 0;                              // a state word is only ever made here; this keeps the shifts in range anyway
  Bits B;
  bits_open(B, stream, r, pos);
  uint32_t nstart = 0, ndone = 0, done_pos = pos, err = 0, err_done = 0, d0 = 0, d1 = 0, d2 = 0;
  for (uint32_t trip = 0; trip < maxtrips && pos < end; ++trip) {
    const int comp = (int)(L.layout >> (6 * blk)) & 3;
    const bool isdc = k == 0;
    const Sym y = next_symbol(B, table_of(L, tabs, comp, isdc));
    pos += (uint32_t)y.len;
    if (y.bad) {                                           // one bit skipped, the state stays
      err = 1;
      continue;
    }
    int rr = y.rr;
    if (isdc && rr) {
      err = 1;
      rr = 0;
    }
    nstart += isdc ? 1u : 0u;
    d0 += (isdc && comp == 0) ? (uint32_t)y.val : 0u;
    d1 += (isdc && comp == 1) ? (uint32_t)y.val : 0u;
    d2 += (isdc && comp == 2) ? (uint32_t)y.val : 0u;
    const bool wr = isdc || y.s != 0;
    int kk = isdc ? 0 : k + rr;
    if (wr && kk > 63) {
      err = 1;
      kk = 63;
    }
    k = wr ? kk + 1 : (rr == 15 ? k + 16 : 64);
    if (k >= 64) {
      k = 0;
      blk = blk + 1 == L.nblk ? 0 : blk + 1;
      ++ndone;
      done_pos = pos;
      err_done = err;
    }
  }
  if (pos > r.nbytes * 8u) err = 1;
  rec->nstart = nstart;
  rec->ndone = ndone;
  rec->done_pos = done_pos;
  rec->err = (err ? ERR_ANY : 0u) | (err_done ? ERR_DONE : 0u);
  rec->dc[0] = d0;
  rec->dc[1] = d1;
  rec->dc[2] = d2;
  rec->_pad = 0;
  return pack_state(pos, k, blk);
}

__host__ __device__ inline uint32_t seg_end(const rgbnm_jpeg_run& r, uint32_t j, int seg_bits) {
  const uint64_t e = ((uint64_t)j + 1) * (uint64_t)seg_bits, total = (uint64_t)r.nbytes * 8u;
  return (uint32_t)(e < total ? e : total);
}
__host__ __device__ inline uint64_t seg_first_state(uint32_t j, int seg_bits) { return pack_state(j * (uint32_t)seg_bits, 0, 0); }

// verify, the part per segment.  done_before: blocks completed in the run's segments before this one; N = nmcu * nblk.
// 0: before the run's last block, nothing wrong; 1: wrong (the run fails); 2: the last block completes here and all is well;
// 3: behind the last block (only padding bits: ignored).
__host__ __device__ inline int seg_verdict(const SegRec& c, uint64_t done_before, uint64_t N, uint32_t total_bits) {
  if (done_before >= N) return 3;
  const uint64_t incl = done_before + c.ndone;
  if (incl < N) return (c.err & ERR_ANY) ? 1 : 0;
  if (incl > N || (c.err & ERR_DONE) || c.done_pos > total_bits || total_bits - c.done_pos > 8u) return 1;
  return 2;
}

// write: segment j's share of the blocks.  tile: as for decode_run, zero on entry and on return.  Returns 0, or -1 when the walk met
// what verify should have excluded (the caller sends the image to the one-lane walk).
// CROP (a compile-time choice, as in decode_run: the plain walk carries no trace of it): the blocks go through flush_block_crop into
// the packed crop `box`, and g is not looked at.
template <bool CROP = false>
__host__ __device__ inline int write_walk(const uint8_t* stream, const rgbnm_jpeg_run& r, const Lane& L, const rgbnm_jpeg_hufftab* tabs,
                                          const uint8_t* zz, const Out& g, int16_t* tile, uint64_t state, uint32_t end, uint32_t maxtrips,
                                          const SegScan& sc, const jpegwalk::Crop box = jpegwalk::Crop()) {
  const uint32_t total_bits = r.nbytes * 8u, N = (uint32_t)r.nmcu * (uint32_t)L.nblk;
  uint32_t pos = state_pos(state), b = sc.b0;
  int k = state_k(state), blk = state_blk(state);
  if (blk >= L.nblk) return -1;
  bool skipping = k != 0;                                  // the block under way at the entry belongs to the segment it started in
  uint32_t p0 = sc.p[0], p1 = sc.p[1], p2 = sc.p[2];
  uint32_t mcu = (uint32_t)r.mcu0 + b / (uint32_t)L.nblk;
  int bi = (int)(b % (uint32_t)L.nblk), mx = (int)(mcu % (uint32_t)L.mcus_x), my = (int)(mcu / (uint32_t)L.mcus_x);
  Bits B;
  bits_open(B, stream, r, pos);
  bool fail = false;
  for (uint32_t trip = 0; trip < maxtrips; ++trip) {
    const bool isdc = k == 0;
    if ((isdc || skipping) && (pos >= end || b >= N)) break;   // nothing more starts here, or only padding bits are left
    if (isdc && bi != blk) {
      fail = true;
      break;
    }
    const int comp = (int)(L.layout >> (6 * blk)) & 3;
    const Sym y = next_symbol(B, table_of(L, tabs, comp, isdc));
    pos += (uint32_t)y.len;
    if (y.bad || (isdc && y.rr) || pos > total_bits) {
      fail = true;
      break;
    }
    p0 += (isdc && comp == 0) ? (uint32_t)y.val : 0u;
    p1 += (isdc && comp == 1) ? (uint32_t)y.val : 0u;
    p2 += (isdc && comp == 2) ? (uint32_t)y.val : 0u;
    const uint32_t dc = comp == 0 ? p0 : comp == 1 ? p1 : p2;
    const bool wr = isdc || y.s != 0;
    const int kk = isdc ? 0 : k + y.rr;
    if (wr && kk > 63) {
      fail = true;
      break;
    }
    if (wr && !skipping) tile[zz[kk]] = (int16_t)(isdc ? (int32_t)dc : y.val);
    k = wr ? kk + 1 : (y.rr == 15 ? k + 16 : 64);
    if (k >= 64) {
      k = 0;
      if (!skipping) {
        if (CROP) jpegwalk::flush_block_crop(tile, box, L, blk, mx, my);
        else jpegwalk::flush_block(tile, g, L, r.image, blk, mx, my);
        ++b;
        jpegwalk::next_block(L, bi, mx, my);
      }
      skipping = false;
      blk = blk + 1 == L.nblk ? 0 : blk + 1;
    }
  }
  if (fail || (k != 0 && !skipping)) {                     // a block half written: the tile goes back to zero
    jpegwalk::zero_tile(tile);
    return -1;
  }
  return 0;
}

// A one-component file's zero chroma: segment j of nseg takes its part of the run's share (jpegwalk::zero_chroma_share).
__host__ __device__ inline void zero_chroma_part(const Out& g, int image, uint32_t mcu0, uint32_t nmcu, uint32_t total, uint32_t j, uint32_t nseg) {
  if (!g.C) return;
  const jpegwalk::Pieces run = jpegwalk::chroma_share(jpegwalk::chroma_pieces(g), mcu0, nmcu, total);
  const jpegwalk::Pieces seg = {run.lo + (run.hi - run.lo) * j / nseg, run.lo + (run.hi - run.lo) * ((uint64_t)j + 1) / nseg};
  jpegwalk::zero_pieces(jpegwalk::chroma_slot(g, image), seg);
}

// ---- the crop form (rgbnm_jpeg_decode_batch_split_crop): the write pass walks only the segments that hold a block of the box ----------
// Scout, sync and verify see the whole run whatever the box.  Behind verify's scan every segment knows the blocks that start in it,
// [b0, b0 + nstart): a raster range of MCUs.  A segment is LIVE iff one of those MCUs holds a block of the box of some component (the
// box mapped through the sampling factors, as jpegwalk::crop_mcus maps it).  The wave that verifies a run counts its live segments,
// reserves that many entries of one list with ONE atomic add and writes the live slots there in segment order; the write launch runs
// over the list, so its waves are dense whatever the boxes.  The order of the runs in the list is the order of the atomics and may
// differ from call to call; the outputs do not depend on it, because every block of a box starts in exactly one segment and that
// segment alone stores it.  The list, its count and the per-run ranges are device data like every other record: a write lane clamps
// the count, re-checks its slot as every segment lane does, and uses the range only to share out a one-component file's zero chroma.
struct RunLive { uint32_t first, count; };                 // the run's entries of the list: [first, first + count)
struct Compact {
  uint32_t* list;       // [nslots]: the live slots, run after run
  RunLive* live;        // [nruns]
  uint32_t* count;      // entries reserved so far
};
// the crop form's scratch: the split call's, then the list, the ranges and the counter.  0 where scratch_bytes gives 0.
inline size_t crop_scratch_bytes(size_t stream_bytes, int nruns, int seg_bits) {
  const size_t base = scratch_bytes(stream_bytes, nruns, seg_bits);
  if (!base) return 0;
  return align16(base) + align16(slot_count(stream_bytes, nruns, seg_bits) * 4) + align16((size_t)nruns * sizeof(RunLive)) + 16;
}
inline Compact carve_crop(void* mem, size_t stream_bytes, int nruns, int seg_bits) {
  uint8_t* p = static_cast<uint8_t*>(mem) + align16(scratch_bytes(stream_bytes, nruns, seg_bits));
  Compact x;
  x.list = reinterpret_cast<uint32_t*>(p); p += align16(slot_count(stream_bytes, nruns, seg_bits) * 4);
  x.live = reinterpret_cast<RunLive*>(p); p += align16((size_t)nruns * sizeof(RunLive));
  x.count = reinterpret_cast<uint32_t*>(p);
  return x;
}

// The live test, closed form: the blocks [b0, b0 + nstart) of the run, cut to its nmcu * nblk, lie in the MCUs [lo, hi] (raster
// order); per component the MCUs that hold a block of its box are a rectangle, and the first MCU of the rectangle at or behind lo is
// found without a loop.
__host__ __device__ inline bool seg_is_live(const rgbnm_jpeg_run& r, const Lane& L, const jpegwalk::Crop& B, uint32_t b0, uint32_t nstart) {
  const uint32_t N = (uint32_t)r.nmcu * (uint32_t)L.nblk;   // below 2^25: check_run
  if (b0 >= N || nstart == 0) return false;
  const uint32_t end = nstart < N - b0 ? b0 + nstart : N, nblk = (uint32_t)L.nblk;
  const int mcus_x = L.mcus_x;
  const int lo = r.mcu0 + (int)(b0 / nblk), hi = r.mcu0 + (int)((end - 1) / nblk);
  for (int c = 0; c < L.ncomp; ++c) {
    const int hs = (int)(L.hv >> (8 * c)) & 15, vs = (int)(L.hv >> (8 * c + 4)) & 15;
    const int t = c ? B.top / 2 : B.top, l = c ? B.left / 2 : B.left, h = c ? B.h / 2 : B.h, w = c ? B.w / 2 : B.w;
    const int x0 = l / hs, xe = (l + w - 1) / hs, x1 = xe < mcus_x ? xe : mcus_x - 1, y0 = t / vs, y1 = (t + h - 1) / vs;
    int y = lo / mcus_x, x = lo - y * mcus_x;
    if (y < y0) {
      y = y0;
      x = x0;
    } else if (x < x0) {
      x = x0;
    } else if (x > x1) {
      ++y;
      x = x0;
    }
    if (x0 <= x1 && y <= y1 && y * mcus_x + x <= hi) return true;
  }
  return false;
}

// Does a run's range of `total` entries from `first` fit the list?  (It always does: a slot is listed at most once.  A run whose
// range does not fit is sent to the one-lane walk.)
__host__ __device__ inline bool list_fits(uint32_t first, uint32_t total, uint32_t nslots) { return first <= nslots && total <= nslots - first; }

// A one-component file's zero chroma in the packed crop: live segment `rank` of the run's `count` takes its part of the run's share
// (jpegwalk::zero_chroma_share_crop).  A split run without a live segment leaves its share to the last launch.
__host__ __device__ inline void zero_chroma_part_crop(const jpegwalk::Crop& B, uint32_t mcu0, uint32_t nmcu, uint32_t total, uint32_t rank,
                                                      uint32_t count) {
  const jpegwalk::Pieces run = jpegwalk::chroma_share((uint64_t)2 * (uint64_t)(B.h / 2) * (uint64_t)(B.w / 2) * 8u, mcu0, nmcu, total);
  const jpegwalk::Pieces seg = {run.lo + (run.hi - run.lo) * rank / count, run.lo + (run.hi - run.lo) * ((uint64_t)rank + 1) / count};
  jpegwalk::zero_pieces(B.C, seg);
}

}  // namespace jpegsplit
