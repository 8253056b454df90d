// Entropy decoding of baseline JPEG files on the device (include/rgbnm.h: rgbnm_jpeg_prepare, rgbnm_jpeg_decode_batch).
//
// The host finds the independent bit streams ("runs": the scan, or one per restart interval) -- jpeg_scan.h, a byte scan -- and the
// kernel below walks them, ONE LANE PER RUN, grid-strided over the run records (1 to 64 runs per wave, see lanes_per_wave).  The walk
// itself is jpeg_walk.h, shared with the stand-alone host checks.  What this file adds is the wave's side of it: wave_tile opens
// the three wave kernels, stage_tables stages the tables for the split passes (the one-lane kernels keep that text written out).
//   - workgroup = one wave of 64 lanes; each lane owns a 128-byte block tile in LDS (pitch 144 bytes, so that the 16-byte moves stay
//     aligned and neighbouring lanes start 36 banks apart).  The walk scatters 2-byte coefficients into the tile; a finished block
//     leaves as eight 16-byte stores -- whole 128-byte lines, zeros included, so no fill launch precedes the kernel -- and the tile
//     is zeroed by the same pass.
//   - the Huffman tables (1440 bytes each in look-up form) are staged in LDS when every live lane of the wave uses the same six
//     (DC / AC per component), which is the common case: a dataset written by one encoder carries the four standard tables in every
//     file.  Otherwise the lanes read the batch's table array in global memory.  The choice is wave-uniform.
//   - an error lowers status[image] with atomicMin; no lane waits for another, no loop depends on the data for its bound.
// decode_crop_kernel is the same launch for a crop box per image (rgbnm_jpeg_decode_batch_crop): runs outside the box are skipped,
// the others stop after the last MCU the box needs, and only the box is stored, packed.  rgbnm_jpeg_decode_batch_split_crop is the
// split decode for such boxes: its verify, write and one-lane launches are kernels of their own behind the split kernels.
#include "common.h"
#include "jpeg_scan.h"
#include "jpeg_walk.h"
#include "jpeg_split.h"
#include "../../include/rgbnm.h"

namespace jpegdec {

constexpr int LANES = 64;
constexpr int PITCH = 144;                 // bytes between the tiles of neighbouring lanes
constexpr int SLOTS = 6;                   // staged tables: slot 2 c = DC of component c, 2 c + 1 = AC
constexpr int MAX_WGS = 4096;
constexpr int TAB_PIECES = (int)(sizeof(rgbnm_jpeg_hufftab) / 16);

__device__ const uint8_t d_zigzag[64] = {JPEGSCAN_ZIGZAG_VALUES};

// A wave kernel's opening: the lane's tile inside s_tile (LANES * PITCH bytes), zeroed, and the zig-zag table in s_zz, behind a
// barrier.  TILE = false (the split passes that store nothing): neither is set up and every lane gets s_tile itself.
template <bool TILE = true>
__device__ __forceinline__ int16_t* wave_tile(uint8_t* s_tile, uint8_t* s_zz) {
  const int lane = threadIdx.x;
  int16_t* tile = reinterpret_cast<int16_t*>(s_tile + (TILE ? lane * PITCH : 0));
  if (TILE) {
    s_zz[lane] = d_zigzag[lane];
    jpegwalk::zero_tile(tile);
  }
  __syncthreads();
  return tile;
}

// One table set for the live lanes of the wave?  Then their six tables go to s_tab (SLOTS entries) between two barriers and the
// result is true: those lanes walk with staged(L) behind s_tab.  Every lane of the wave calls this, live or not.
__device__ __forceinline__ bool stage_tables(bool live, const jpegwalk::Lane& L, const rgbnm_jpeg_hufftab* tables, rgbnm_jpeg_hufftab* s_tab) {
  using jpegwalk::V16;
  const unsigned long long mask = __ballot(live);
  if (mask == 0) return false;
  const int lane = threadIdx.x, first = __ffsll((long long)mask) - 1;
  const uint64_t dc0 = __shfl((unsigned long long)L.dcsel, first, LANES), ac0 = __shfl((unsigned long long)L.acsel, first, LANES);
  if (!__all(!live || (L.dcsel == dc0 && L.acsel == ac0))) return false;
  __syncthreads();                         // the previous round's readers of s_tab are done
  for (int j = lane; j < SLOTS * TAB_PIECES; j += LANES) {
    const int slot = j / TAB_PIECES, piece = j - slot * TAB_PIECES;
    const uint32_t t = (uint32_t)(((slot & 1) ? ac0 : dc0) >> (16 * (slot >> 1))) & 0xFFFFu;   // < ntables: check_run
    reinterpret_cast<V16*>(&s_tab[slot])[piece] = reinterpret_cast<const V16*>(&tables[t])[piece];
  }
  __syncthreads();
  return true;
}
// the lane record whose table indices are the staged slots
__device__ __forceinline__ jpegwalk::Lane staged(jpegwalk::Lane L) {
  L.dcsel = 0ull | (2ull << 16) | (4ull << 32);
  L.acsel = 1ull | (3ull << 16) | (5ull << 32);
  return L;
}

struct Args {
  rgbnm_jpeg_device_plan p;
  jpegwalk::Out g;
  int32_t* status;
  int lanes;                               // runs per wave, 1..64
  // the split call's last launch (rgbnm_jpeg_decode_batch_split; NULL in the plain call): a split run whose image the segment
  // lanes have written (path == 1) is left alone
  const jpegsplit::RunInfo* info;
  const int32_t* path;
};

__global__ __launch_bounds__(LANES) void decode_kernel(Args a) {
  using namespace jpegwalk;
  __shared__ alignas(16) uint8_t s_tile[LANES * PITCH];
  __shared__ alignas(16) rgbnm_jpeg_hufftab s_tab[SLOTS];
  __shared__ uint8_t s_zz[64];
  const int lane = threadIdx.x;
  int16_t* tile = wave_tile(s_tile, s_zz);
  const int nruns = a.p.nruns, per = a.lanes;
  for (long long base = (long long)blockIdx.x * per; base < nruns; base += (long long)gridDim.x * per) {
    const int ri = (int)base + lane;
    bool live = lane < per && ri < nruns;
    rgbnm_jpeg_run r = {};
    Lane L = {};
    if (live) {
      r = a.p.runs[ri];
      if (r.nmcu == 0) {                   // the record of a file the host refused
        live = false;
      } else if (check_run(r, a.p.images, a.g.n, a.p.stream_bytes, a.p.ntables, &L) != 0) {
        live = false;
        if (r.image >= 0 && r.image < a.g.n) atomicMin(&a.status[r.image], RGBNM_JPEG_ERECORD);
      } else if (a.info && a.info[ri].nseg && a.path[r.image] == 1) {
        live = false;
      }
    }
    // One table set for the whole wave?  Written out, not stage_tables: with the helper the launches on files with a restart marker
    // per MCU row measured 1 - 3 % slower (crop: more), against a run-to-run disagreement below 1 %.  Two calls of the walk, not one
    // behind `shared ? s_tab : tables`: that pointer would lose its address space and every table read become a flat load.
    int err = 0;
    const unsigned long long mask = __ballot(live);
    if (mask == 0) continue;
    const int first = __ffsll((long long)mask) - 1;
    const uint64_t dc0 = __shfl((unsigned long long)L.dcsel, first, LANES), ac0 = __shfl((unsigned long long)L.acsel, first, LANES);
    const bool shared = __all(!live || (L.dcsel == dc0 && L.acsel == ac0));
    if (shared) {
      __syncthreads();                     // the previous round's readers of s_tab are done
      for (int j = lane; j < SLOTS * TAB_PIECES; j += LANES) {
        const int slot = j / TAB_PIECES, piece = j - slot * TAB_PIECES;
        const uint32_t t = (uint32_t)(((slot & 1) ? ac0 : dc0) >> (16 * (slot >> 1))) & 0xFFFFu;   // < ntables: check_run
        reinterpret_cast<V16*>(&s_tab[slot])[piece] = reinterpret_cast<const V16*>(&a.p.tables[t])[piece];
      }
      __syncthreads();
      if (live) err = decode_run(a.p.stream, r, staged(L), s_tab, s_zz, a.g, tile);
    } else if (live) {
      err = decode_run(a.p.stream, r, L, a.p.tables, s_zz, a.g, tile);
    }
    if (live) {
      if (err) atomicMin(&a.status[r.image], err);
      if (L.ncomp == 1) zero_chroma_share(a.g, r.image, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
    }
  }
}

// ---- the crop decode (rgbnm_jpeg_decode_batch_crop): decode_kernel's structure around the crop form of the walk ---------------------
// A lane first decides, from its image's box, how many MCUs of its run it has to walk (jpeg_walk.h, crop_mcus): none -- it is then
// as idle as the lane of a refused record, and does not count when the wave decides whether to stage the tables -- or up to the last
// MCU that holds a block of the box.
struct CArgs {
  rgbnm_jpeg_device_plan p;
  int n, Hb, Wb, Hbc, Wbc;
  const int32_t* boxes;                    // [n][4]
  const long long* y_off;                  // [n]
  const long long* c_off;
  int16_t* Y;                              // packed, y_elems
  int16_t* C;                              // packed, c_elems
  size_t y_elems, c_elems;
  int32_t* status;
  uint32_t* walked;                        // [nruns] or NULL
  int lanes;
};

__global__ __launch_bounds__(LANES) void decode_crop_kernel(CArgs a) {
  using namespace jpegwalk;
  __shared__ alignas(16) uint8_t s_tile[LANES * PITCH];
  __shared__ alignas(16) rgbnm_jpeg_hufftab s_tab[SLOTS];
  __shared__ uint8_t s_zz[64];
  const int lane = threadIdx.x;
  int16_t* tile = wave_tile(s_tile, s_zz);
  const int nruns = a.p.nruns, per = a.lanes;
  for (long long base = (long long)blockIdx.x * per; base < nruns; base += (long long)gridDim.x * per) {
    const int ri = (int)base + lane;
    const bool mine = lane < per && ri < nruns;
    bool ok = mine;                        // the records and the box passed: the run's image is written by this call
    rgbnm_jpeg_run r = {};
    Lane L = {};
    Crop B = {};
    uint32_t nwalk = 0;
    if (ok) {
      r = a.p.runs[ri];
      if (r.nmcu == 0) {                   // the record of a file the host refused
        ok = false;
      } else if (check_run(r, a.p.images, a.n, a.p.stream_bytes, a.p.ntables, &L) != 0) {
        ok = false;
        if (r.image >= 0 && r.image < a.n) atomicMin(&a.status[r.image], RGBNM_JPEG_ERECORD);
      } else if (check_box(a.boxes + 4 * (size_t)r.image, a.y_off[r.image], a.c_off[r.image], a.Hb, a.Wb, a.Hbc, a.Wbc, a.Y, a.y_elems, a.C,
                           a.c_elems, &B) != 0) {
        ok = false;
        atomicMin(&a.status[r.image], RGBNM_JPEG_EBOX);
      } else {
        nwalk = crop_mcus(r, L, B);
      }
    }
    const bool live = nwalk != 0;          // only these lanes walk
    int err = 0;                           // staging written out and two calls of the walk: as in decode_kernel
    const unsigned long long mask = __ballot(live);
    if (mask != 0) {
      const int first = __ffsll((long long)mask) - 1;
      const uint64_t dc0 = __shfl((unsigned long long)L.dcsel, first, LANES), ac0 = __shfl((unsigned long long)L.acsel, first, LANES);
      const bool shared = __all(!live || (L.dcsel == dc0 && L.acsel == ac0));
      if (shared) {
        __syncthreads();                   // the previous round's readers of s_tab are done
        for (int j = lane; j < SLOTS * TAB_PIECES; j += LANES) {
          const int slot = j / TAB_PIECES, piece = j - slot * TAB_PIECES;
          const uint32_t t = (uint32_t)(((slot & 1) ? ac0 : dc0) >> (16 * (slot >> 1))) & 0xFFFFu;   // < ntables: check_run
          reinterpret_cast<V16*>(&s_tab[slot])[piece] = reinterpret_cast<const V16*>(&a.p.tables[t])[piece];
        }
        __syncthreads();
        if (live) err = decode_run_crop(a.p.stream, r, staged(L), s_tab, s_zz, B, nwalk, tile);
      } else if (live) {
        err = decode_run_crop(a.p.stream, r, L, a.p.tables, s_zz, B, nwalk, tile);
      }
    }
    if (err) atomicMin(&a.status[r.image], err);
    // a skipped run takes its share of a one-component file's zero chroma like a walked one
    if (ok && L.ncomp == 1) zero_chroma_share_crop(B, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
    if (mine && a.walked) a.walked[ri] = nwalk;
  }
}

// ---- the split decode (jpeg_split.h): one lane per bit segment of a run -----------------------------------------------------------
// Launches, in stream order: init, map, scout, `rounds` x sync, verify, write, then decode_kernel for what is left.  Their number
// depends on the arguments only.  A lane reads its predecessor's exit from the buffer the launch BEFORE wrote, never from its own.
// One exception, harmless: a write lane whose walk fails raises path[image] to 2 while other write lanes of the launch read it; whichever
// value they see, the one-lane kernel behind them rewrites that whole image.
struct SArgs {
  rgbnm_jpeg_device_plan p;
  jpegwalk::Out g;
  int32_t* path;
  jpegsplit::Scratch s;
  int seg_bits, min_seg, cur, lanes;       // cur: the exit buffer to read (sync), the final one (verify)
};

__global__ __launch_bounds__(256) void split_init_kernel(SArgs a) {
  const size_t m = a.s.nslots > (uint32_t)a.g.n ? a.s.nslots : (size_t)a.g.n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) {
    if (i < a.s.nslots) a.s.seg_run[i] = -1;
    if (i < (size_t)a.g.n) a.path[i] = 0;
  }
}

// one wave per run: is it split, where do its segments go
__global__ __launch_bounds__(LANES) void split_map_kernel(SArgs a) {
  using namespace jpegsplit;
  const int lane = threadIdx.x;
  for (int ri = blockIdx.x; ri < a.p.nruns; ri += gridDim.x) {
    const rgbnm_jpeg_run r = a.p.runs[ri];
    Lane L;
    RunInfo info = {0u, 0u};
    if (r.nmcu != 0 && jpegwalk::check_run(r, a.p.images, a.g.n, a.p.stream_bytes, a.p.ntables, &L) == 0)
      info = map_run(r, ri, a.seg_bits, a.min_seg, a.s.nslots);
    if (lane == 0) {
      a.s.info[ri] = info;
      if (info.nseg) atomicMax(&a.path[r.image], 1);
    }
    for (uint32_t j = lane; j < info.nseg; j += LANES) a.s.seg_run[info.base + j] = ri;
  }
}

// MODE 0 scout, 1 sync, 2 write.  Workgroup = one wave; lanes = consecutive slots, so normally consecutive segments of one run, and
// the tables are staged as in decode_kernel; the walks here are one call each behind a generic table pointer.
template <int MODE>
__global__ __launch_bounds__(LANES) void split_seg_kernel(SArgs a) {
  using namespace jpegsplit;
  __shared__ alignas(16) uint8_t s_tile[MODE == 2 ? LANES * PITCH : 16];
  __shared__ alignas(16) rgbnm_jpeg_hufftab s_tab[SLOTS];
  __shared__ uint8_t s_zz[64];
  const int lane = threadIdx.x;
  int16_t* tile = wave_tile<MODE == 2>(s_tile, s_zz);
  const uint32_t nslots = a.s.nslots;
  const int per = a.lanes, nxt = a.cur ^ 1;
  for (long long base = (long long)blockIdx.x * per; base < (long long)nslots; base += (long long)gridDim.x * per) {
    const uint32_t slot = (uint32_t)base + (uint32_t)lane;
    bool live = lane < per && slot < nslots;
    int ri = -1;
    uint32_t j = 0, nseg = 0;
    rgbnm_jpeg_run r = {};
    Lane L = {};
    if (live) {
      ri = a.s.seg_run[slot];
      live = ri >= 0 && ri < a.p.nruns;
    }
    if (live) {
      const RunInfo info = a.s.info[ri];
      j = slot - info.base;                // unsigned: a slot in front of the run's fails the next test too
      nseg = info.nseg;
      live = j < nseg;
    }
    if (live) {
      r = a.p.runs[ri];
      live = r.nmcu != 0 && jpegwalk::check_run(r, a.p.images, a.g.n, a.p.stream_bytes, a.p.ntables, &L) == 0;
    }
    uint64_t state = 0;
    if (MODE == 0 && live) state = j == 0 ? pack_state(0, 0, 0) : seg_first_state(j, a.seg_bits);
    if (MODE == 1 && live) {               // walk again only where the entry is not the predecessor's exit of the round before
      const uint64_t mine = a.s.exits[a.cur][slot];
      const uint64_t pe = j ? a.s.exits[a.cur][slot - 1] : 0;
      if (j == 0 || a.s.entry[slot] == pe) {
        a.s.exits[nxt][slot] = mine;
        live = false;
      }
      state = pe;
    }
    if (MODE == 2 && live) {
      live = a.path[r.image] == 1;
      state = a.s.entry[slot];
    }
    const rgbnm_jpeg_hufftab* tabs = a.p.tables;
    Lane S = L;
    if (stage_tables(live, L, a.p.tables, s_tab)) {
      tabs = s_tab;
      S = staged(L);
    }
    if (!live) continue;
    const uint32_t end = seg_end(r, j, a.seg_bits);
    if (MODE == 2) {
      const SegScan sc = a.s.scan[slot];
      if (write_walk(a.p.stream, r, S, tabs, s_zz, a.g, tile, state, end, (uint32_t)a.seg_bits + 64u, sc) != 0) atomicMax(&a.path[r.image], 2);
      if (L.ncomp == 1) zero_chroma_part(a.g, r.image, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total, j, nseg);
    } else {
      SegRec rec;
      const uint64_t out = scout_walk(a.p.stream, r, S, tabs, state, end, (uint32_t)a.seg_bits + 1u, &rec);
      a.s.entry[slot] = state;
      a.s.exits[MODE == 0 ? 0 : nxt][slot] = out;
      a.s.rec[slot] = rec;
    }
  }
}

// one wave per split run: converged? complete? and the exclusive scan over its segments (block index and DC predictors at each entry)
__global__ __launch_bounds__(LANES) void split_verify_kernel(SArgs a) {
  using namespace jpegsplit;
  const int lane = threadIdx.x;
  const uint64_t* fin = a.s.exits[a.cur];
  for (int ri = blockIdx.x; ri < a.p.nruns; ri += gridDim.x) {
    const RunInfo info = a.s.info[ri];
    if (info.nseg == 0) continue;
    const rgbnm_jpeg_run r = a.p.runs[ri];
    Lane L;
    if (jpegwalk::check_run(r, a.p.images, a.g.n, a.p.stream_bytes, a.p.ntables, &L) != 0) continue;   // map split it: it passed there
    const uint64_t N = (uint64_t)r.nmcu * (uint64_t)L.nblk;
    const uint32_t total_bits = r.nbytes * 8u;
    uint32_t carry[5] = {0, 0, 0, 0, 0};   // blocks completed, blocks started, DC sums
    bool bad = false, found = false;
    for (uint32_t c0 = 0; c0 < info.nseg; c0 += LANES) {
      const uint32_t j = c0 + (uint32_t)lane, slot = info.base + j;
      const bool v = j < info.nseg;
      SegRec c = {};
      bool conv = true;
      if (v) {
        c = a.s.rec[slot];
        // the slot is this run's (two runs that overlap in the stream would share slots: then the records are not this run's)
        conv = a.s.seg_run[slot] == ri && a.s.entry[slot] == (j ? fin[slot - 1] : pack_state(0, 0, 0));
      }
      const uint32_t own[5] = {c.ndone, c.nstart, c.dc[0], c.dc[1], c.dc[2]};
      uint32_t incl[5];
      for (int q = 0; q < 5; ++q) {
        uint32_t x = own[q];
        for (int d = 1; d < LANES; d <<= 1) {
          const uint32_t y = __shfl_up(x, d, LANES);
          if (lane >= d) x += y;
        }
        incl[q] = x;
      }
      int verdict = 0;
      if (v) {
        verdict = seg_verdict(c, (uint64_t)carry[0] + incl[0] - own[0], N, total_bits);
        SegScan sc;
        sc.b0 = carry[1] + incl[1] - own[1];
        for (int q = 0; q < 3; ++q) sc.p[q] = carry[2 + q] + incl[2 + q] - own[2 + q];
        a.s.scan[slot] = sc;
      }
      bad = bad || __any(!conv || verdict == 1);
      found = found || __any(verdict == 2);
      for (int q = 0; q < 5; ++q) carry[q] += __shfl(incl[q], LANES - 1, LANES);
    }
    if (lane == 0 && (bad || !found)) atomicMax(&a.path[r.image], 2);
  }
}

// ---- the split decode for a crop box per image (rgbnm_jpeg_decode_batch_split_crop; jpeg_split.h, the crop form) ----------------------
// Launches: init, map, scout, `rounds` x sync -- the split call's own kernels, which look at no box -- then verify, write and the
// one-lane launch in the forms below.  Kernels of their own, not switches in the ones above: those stay the code they were.
struct XArgs {
  SArgs s;                                 // s.g: n and the grids; its Y / C are NULL
  const int32_t* boxes;                    // [n][4]
  const long long* y_off;                  // [n]
  const long long* c_off;
  int16_t* Y;                              // packed, y_elems
  int16_t* C;                              // packed, c_elems
  size_t y_elems, c_elems;
  int32_t* status;
  uint32_t* walked;                        // [nruns] or NULL
  uint32_t* seg_live;                      // [nruns] or NULL
  jpegsplit::Compact x;
  int run_lanes;                           // runs per wave of the last launch
  int fixed_lanes;                         // option "jpeg_lanes" is set: the write launch takes s.lanes entries per wave whatever the list's length
};

__device__ __forceinline__ int box_of(const XArgs& a, int image, jpegwalk::Crop* B) {
  return jpegwalk::check_box(a.boxes + 4 * (size_t)image, a.y_off[image], a.c_off[image], a.s.g.Hb, a.s.g.Wb, a.s.g.Hbc, a.s.g.Wbc, a.Y,
                             a.y_elems, a.C, a.c_elems, B);
}

// split_init_kernel, and the list is empty
__global__ __launch_bounds__(256) void split_crop_init_kernel(XArgs a) {
  const size_t m = a.s.s.nslots > (uint32_t)a.s.g.n ? a.s.s.nslots : (size_t)a.s.g.n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) {
    if (i < a.s.s.nslots) a.s.s.seg_run[i] = -1;
    if (i < (size_t)a.s.g.n) a.s.path[i] = 0;
    if (i == 0) *a.x.count = 0;
  }
}

// split_verify_kernel's checks and scan, word for word; the wave also counts the run's live segments on the way and, if the run
// passed, lists them: one atomic add reserves the range, a second trip over the segments fills it in segment order.  A bad box
// leaves the run without live segments (the last launch reports it).
__global__ __launch_bounds__(LANES) void split_verify_crop_kernel(XArgs a) {
  using namespace jpegsplit;
  const int lane = threadIdx.x;
  const uint64_t* fin = a.s.s.exits[a.s.cur];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int ri = blockIdx.x; ri < a.s.p.nruns; ri += gridDim.x) {
    const RunInfo info = a.s.s.info[ri];
    const rgbnm_jpeg_run r = a.s.p.runs[ri];
    Lane L;
    if (info.nseg == 0 || jpegwalk::check_run(r, a.s.p.images, a.s.g.n, a.s.p.stream_bytes, a.s.p.ntables, &L) != 0) {
      if (lane == 0) a.x.live[ri] = RunLive{0u, 0u};
      continue;
    }
    jpegwalk::Crop B = {};
    const bool boxed = box_of(a, r.image, &B) == 0;
    const uint64_t N = (uint64_t)r.nmcu * (uint64_t)L.nblk;
    const uint32_t total_bits = r.nbytes * 8u;
    uint32_t carry[5] = {0, 0, 0, 0, 0};   // blocks completed, blocks started, DC sums
    uint32_t nlive = 0;
    bool bad = false, found = false;
    for (uint32_t c0 = 0; c0 < info.nseg; c0 += LANES) {
      const uint32_t j = c0 + (uint32_t)lane, slot = info.base + j;
      const bool v = j < info.nseg;
      SegRec c = {};
      bool conv = true;
      if (v) {
        c = a.s.s.rec[slot];
        conv = a.s.s.seg_run[slot] == ri && a.s.s.entry[slot] == (j ? fin[slot - 1] : pack_state(0, 0, 0));
      }
      const uint32_t own[5] = {c.ndone, c.nstart, c.dc[0], c.dc[1], c.dc[2]};
      uint32_t incl[5];
      for (int q = 0; q < 5; ++q) {
        uint32_t x = own[q];
        for (int d = 1; d < LANES; d <<= 1) {
          const uint32_t y = __shfl_up(x, d, LANES);
          if (lane >= d) x += y;
        }
        incl[q] = x;
      }
      int verdict = 0;
      bool lv = false;
      if (v) {
        verdict = seg_verdict(c, (uint64_t)carry[0] + incl[0] - own[0], N, total_bits);
        SegScan sc;
        sc.b0 = carry[1] + incl[1] - own[1];
        for (int q = 0; q < 3; ++q) sc.p[q] = carry[2 + q] + incl[2 + q] - own[2 + q];
        a.s.s.scan[slot] = sc;
        lv = boxed && seg_is_live(r, L, B, sc.b0, c.nstart);
      }
      bad = bad || __any(!conv || verdict == 1);
      found = found || __any(verdict == 2);
      nlive += (uint32_t)__popcll(__ballot(lv));
      for (int q = 0; q < 5; ++q) carry[q] += __shfl(incl[q], LANES - 1, LANES);
    }
    bool passed = !(bad || !found);
    uint32_t first = 0;
    if (passed && nlive) {
      if (lane == 0) first = atomicAdd(a.x.count, nlive);
      first = __shfl(first, 0, LANES);
      if (!list_fits(first, nlive, a.s.s.nslots)) passed = false;
    }
    if (!passed) nlive = 0;
    if (lane == 0) {
      if (!passed) atomicMax(&a.s.path[r.image], 2);
      a.x.live[ri] = RunLive{first, nlive};
    }
    uint32_t at = first;
    for (uint32_t c0 = 0; nlive && c0 < info.nseg; c0 += LANES) {
      const uint32_t j = c0 + (uint32_t)lane, slot = info.base + j;
      const bool lv = j < info.nseg && seg_is_live(r, L, B, a.s.s.scan[slot].b0, a.s.s.rec[slot].nstart);   // this lane's own words
      const unsigned long long m = __ballot(lv);
      const uint32_t k = at + (uint32_t)__popcll(m & below);
      if (lv && k - first < nlive) a.x.list[k] = slot;
      at += (uint32_t)__popcll(m);
    }
  }
}

// split_seg_kernel<2> over the list of live slots: lanes = consecutive entries, so normally live segments of one run.  The count and
// every entry are re-checked as a slot's run is in every segment launch.
__global__ __launch_bounds__(LANES) void split_write_crop_kernel(XArgs a) {
  using namespace jpegsplit;
  __shared__ alignas(16) uint8_t s_tile[LANES * PITCH];
  __shared__ alignas(16) rgbnm_jpeg_hufftab s_tab[SLOTS];
  __shared__ uint8_t s_zz[64];
  const int lane = threadIdx.x;
  int16_t* tile = wave_tile(s_tile, s_zz);
  const uint32_t nslots = a.s.s.nslots, listed = *a.x.count, nlist = listed < nslots ? listed : nslots;
  // lanes_per_wave's rule on the list's length, which only the device knows: about 2048 waves first, fuller waves beyond that
  const uint32_t spread = (nlist + 2047u) / 2048u;
  const int per = a.fixed_lanes ? a.s.lanes : (int)(spread < 1u ? 1u : spread > (uint32_t)LANES ? (uint32_t)LANES : spread);
  const jpegwalk::Out none = {0, 0, 0, 0, 0, nullptr, nullptr};
  for (long long base = (long long)blockIdx.x * per; base < (long long)nlist; base += (long long)gridDim.x * per) {
    const uint32_t at = (uint32_t)base + (uint32_t)lane;
    bool live = lane < per && at < nlist;
    uint32_t slot = 0, j = 0;
    int ri = -1;
    rgbnm_jpeg_run r = {};
    Lane L = {};
    jpegwalk::Crop B = {};
    if (live) {
      slot = a.x.list[at];
      live = slot < nslots;
    }
    if (live) {
      ri = a.s.s.seg_run[slot];
      live = ri >= 0 && ri < a.s.p.nruns;
    }
    if (live) {
      const RunInfo info = a.s.s.info[ri];
      j = slot - info.base;                // unsigned: a slot in front of the run's fails the next test too
      live = j < info.nseg;
    }
    if (live) {
      r = a.s.p.runs[ri];
      live = r.nmcu != 0 && jpegwalk::check_run(r, a.s.p.images, a.s.g.n, a.s.p.stream_bytes, a.s.p.ntables, &L) == 0;
    }
    if (live) live = a.s.path[r.image] == 1;
    if (live && box_of(a, r.image, &B) != 0) {
      live = false;
      atomicMin(&a.status[r.image], RGBNM_JPEG_EBOX);
    }
    const rgbnm_jpeg_hufftab* tabs = a.s.p.tables;
    Lane S = L;
    if (stage_tables(live, L, a.s.p.tables, s_tab)) {
      tabs = s_tab;
      S = staged(L);
    }
    if (!live) continue;
    const SegScan sc = a.s.s.scan[slot];
    if (write_walk<true>(a.s.p.stream, r, S, tabs, s_zz, none, tile, a.s.s.entry[slot], seg_end(r, j, a.s.seg_bits), (uint32_t)a.s.seg_bits + 64u,
                         sc, B) != 0)
      atomicMax(&a.s.path[r.image], 2);
    if (L.ncomp == 1) {
      const RunLive rl = a.x.live[ri];
      if (at - rl.first < rl.count) zero_chroma_part_crop(B, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total, at - rl.first, rl.count);
    }
  }
}

// decode_crop_kernel's walk for what is left: the runs that were not split and every run of an image whose split did not pass.  A split
// run of a path 1 image is left alone as decode_kernel leaves it under the split call -- but its box is checked here too (a bad box
// gave it no live segment, so no write lane has reported it), and a one-component run without a live segment zeroes its share of the
// chroma crop here.  seg_live is written here, where the image's final path is known.
__global__ __launch_bounds__(LANES) void decode_crop_rest_kernel(XArgs a) {
  using namespace jpegwalk;
  __shared__ alignas(16) uint8_t s_tile[LANES * PITCH];
  __shared__ alignas(16) rgbnm_jpeg_hufftab s_tab[SLOTS];
  __shared__ uint8_t s_zz[64];
  const int lane = threadIdx.x;
  int16_t* tile = wave_tile(s_tile, s_zz);
  const int nruns = a.s.p.nruns, per = a.run_lanes, n = a.s.g.n;
  for (long long base = (long long)blockIdx.x * per; base < nruns; base += (long long)gridDim.x * per) {
    const int ri = (int)base + lane;
    const bool mine = lane < per && ri < nruns;
    bool ok = mine;                        // the records and the box passed: the run's image is written by this call
    rgbnm_jpeg_run r = {};
    Lane L = {};
    Crop B = {};
    uint32_t nwalk = 0, nlive = 0;
    if (ok) {
      r = a.s.p.runs[ri];
      if (r.nmcu == 0) {                   // the record of a file the host refused
        ok = false;
      } else if (check_run(r, a.s.p.images, n, a.s.p.stream_bytes, a.s.p.ntables, &L) != 0) {
        ok = false;
        if (r.image >= 0 && r.image < n) atomicMin(&a.status[r.image], RGBNM_JPEG_ERECORD);
      } else if (box_of(a, r.image, &B) != 0) {
        ok = false;
        atomicMin(&a.status[r.image], RGBNM_JPEG_EBOX);
      } else if (a.s.s.info[ri].nseg && a.s.path[r.image] == 1) {      // the segment lanes have written it
        const jpegsplit::RunLive rl = a.x.live[ri];
        nlive = rl.count;
        if (L.ncomp == 1 && nlive == 0) zero_chroma_share_crop(B, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
        ok = false;
      } else {
        // a run that was not split, in an image whose split runs passed: walked to its end, so that the image's status is the whole
        // decode's (verify has vouched for the split runs; a walk that stops early vouches for nothing behind the box)
        nwalk = a.s.path[r.image] == 1 ? (uint32_t)r.nmcu : crop_mcus(r, L, B);
      }
    }
    const bool live = nwalk != 0;          // only these lanes walk
    int err = 0;
    const rgbnm_jpeg_hufftab* tabs = a.s.p.tables;
    Lane S = L;
    if (stage_tables(live, L, a.s.p.tables, s_tab)) {
      tabs = s_tab;
      S = staged(L);
    }
    if (live) err = decode_run_crop(a.s.p.stream, r, S, tabs, s_zz, B, nwalk, tile);
    if (err) atomicMin(&a.status[r.image], err);
    // a skipped run takes its share of a one-component file's zero chroma like a walked one
    if (ok && L.ncomp == 1) zero_chroma_share_crop(B, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
    if (mine && a.walked) a.walked[ri] = nwalk;
    if (mine && a.seg_live) a.seg_live[ri] = nlive;
  }
}

// ---- the host side of the four entries ------------------------------------------------------------------------------------------------
// What all four refuse: the plan, n, the grids, the outputs and the status and their alignment, and the plan's buffers where it has runs.
static bool bad_call(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, const void* Y, const void* C, const void* status) {
  if (!plan || !Y || !C || !status || n <= 0 || Hb < 1 || Wb < 1 || Hbc < 1 || Wbc < 1 || Hb > 4096 || Wb > 4096 || Hbc > 4096 ||
      Wbc > 4096 || plan->nruns < 0 || plan->ntables < 0)
    return true;
  if (((uintptr_t)Y & 15) || ((uintptr_t)C & 15) || ((uintptr_t)status & 3)) return true;
  return plan->nruns && (!plan->stream || !plan->runs || !plan->images || !plan->tables || ((uintptr_t)plan->stream & 3) ||
                         ((uintptr_t)plan->tables & 15) || ((uintptr_t)plan->runs & 3) || ((uintptr_t)plan->images & 3));
}

// Runs (or segments) per wave.  What is rare for a lane -- a code longer than 9 bits, a refill, the end of a block -- happens in almost
// every trip of a wave whose 64 lanes all walk, and the wave pays for each.  A batch rarely has runs for every SIMD of the device
// (256 without restart markers, 8192 with one per MCU row), so the items are spread over about 2048 waves first and the waves fill
// up only beyond that.  Option "jpeg_lanes" (1..64) fixes the number instead.  (The runs a crop box lets skip are not known here.)
static int lanes_per_wave(long long items) {
  const int opt = rgbnm_get_option("jpeg_lanes");
  const long long per = opt >= 1 && opt <= LANES ? opt : cdivl(items, 2048);
  return (int)(per < 1 ? 1 : per > LANES ? LANES : per);
}

static jpegwalk::Out out_of(int n, int Hb, int Wb, int Hbc, int Wbc, int16_t* Y, int16_t* C) {
  const jpegwalk::Out g = {n, Hb, Wb, Hbc, Wbc, Y, C};
  return g;
}

}  // namespace jpegdec

extern "C" {

int rgbnm_jpeg_prepare(const uint8_t* const* bufs, const size_t* lens, int n, int Hb, int Wb, int Hbc, int Wbc, rgbnm_jpeg_plan* plan) {
  return jpegscan::prepare(bufs, lens, n, Hb, Wb, Hbc, Wbc, plan);
}

int rgbnm_jpeg_decode_batch(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, int16_t* Y, int16_t* CbCr,
                            int32_t* status, void* stream) {
  using namespace jpegdec;
  if (bad_call(plan, n, Hb, Wb, Hbc, Wbc, Y, CbCr, status)) return RGBNM_EINVAL;
  if (plan->nruns == 0) return RGBNM_OK;
  Args a;
  a.p = *plan;
  a.g = out_of(n, Hb, Wb, Hbc, Wbc, Y, CbCr);
  a.status = status;
  a.info = nullptr;
  a.path = nullptr;
  a.lanes = lanes_per_wave(plan->nruns);
  const int groups = cdiv(plan->nruns, a.lanes);
  decode_kernel<<<groups < MAX_WGS ? groups : MAX_WGS, LANES, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

int rgbnm_jpeg_decode_batch_crop(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, const int32_t* boxes,
                                 const long long* y_off, const long long* c_off, int16_t* Ypacked, size_t y_elems, int16_t* Cpacked,
                                 size_t c_elems, int32_t* status, uint32_t* walked, void* stream) {
  using namespace jpegdec;
  if (bad_call(plan, n, Hb, Wb, Hbc, Wbc, Ypacked, Cpacked, status)) return RGBNM_EINVAL;
  if (!boxes || !y_off || !c_off || y_elems == 0 || c_elems == 0) return RGBNM_EINVAL;
  if (((uintptr_t)boxes & 3) || ((uintptr_t)y_off & 7) || ((uintptr_t)c_off & 7) || ((uintptr_t)walked & 3)) return RGBNM_EINVAL;
  if (plan->nruns == 0) return RGBNM_OK;
  CArgs a;
  a.p = *plan;
  a.n = n; a.Hb = Hb; a.Wb = Wb; a.Hbc = Hbc; a.Wbc = Wbc;
  a.boxes = boxes; a.y_off = y_off; a.c_off = c_off;
  a.Y = Ypacked; a.C = Cpacked; a.y_elems = y_elems; a.c_elems = c_elems;
  a.status = status;
  a.walked = walked;
  a.lanes = lanes_per_wave(plan->nruns);
  const int groups = cdiv(plan->nruns, a.lanes);
  decode_crop_kernel<<<groups < MAX_WGS ? groups : MAX_WGS, LANES, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

size_t rgbnm_jpeg_split_scratch_bytes(size_t stream_bytes, int nruns, int seg_bits) {
  return jpegsplit::scratch_bytes(stream_bytes, nruns, seg_bits);
}

int rgbnm_jpeg_decode_batch_split(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, int16_t* Y, int16_t* CbCr,
                                  int32_t* status, int32_t* path, void* scratch, size_t scratch_bytes, int seg_bits, int rounds,
                                  void* stream) {
  using namespace jpegdec;
  if (bad_call(plan, n, Hb, Wb, Hbc, Wbc, Y, CbCr, status)) return RGBNM_EINVAL;
  if (!path || ((uintptr_t)path & 3) || rounds < 0 || rounds > jpegsplit::ROUNDS_MAX) return RGBNM_EINVAL;
  const size_t need = jpegsplit::scratch_bytes(plan->stream_bytes, plan->nruns, seg_bits);   // 0: seg_bits out of range
  if (need == 0 || !scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need) return RGBNM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SArgs s;
  s.p = *plan;
  s.g = out_of(n, Hb, Wb, Hbc, Wbc, Y, CbCr);
  s.path = path;
  s.s = jpegsplit::carve(scratch, plan->stream_bytes, plan->nruns, seg_bits);
  s.seg_bits = seg_bits;
  const int ms = rgbnm_get_option("jpeg_min_seg");
  s.min_seg = ms >= 2 ? ms : jpegsplit::MIN_SEG;
  s.cur = 0;
  // Option "jpeg_split_wgs" caps the workgroups of every launch below (tests: each grid-stride loop goes round again).
  const int cap_opt = rgbnm_get_option("jpeg_split_wgs");
  const int cap = cap_opt >= 1 && cap_opt < MAX_WGS ? cap_opt : MAX_WGS;
  auto grid = [cap](long long groups) { return (unsigned)(groups < 1 ? 1 : groups < cap ? groups : cap); };
  const long long nslots = s.s.nslots;
  split_init_kernel<<<grid(cdivl(nslots > n ? nslots : n, 256)), 256, 0, st>>>(s);
  LAUNCH_CHECK();
  if (plan->nruns == 0) return RGBNM_OK;
  s.lanes = lanes_per_wave(nslots);
  const unsigned seg_grid = grid(cdivl(nslots, s.lanes)), run_grid = grid(plan->nruns);
  split_map_kernel<<<run_grid, LANES, 0, st>>>(s);
  LAUNCH_CHECK();
  split_seg_kernel<0><<<seg_grid, LANES, 0, st>>>(s);
  LAUNCH_CHECK();
  for (int j = 0; j < rounds; ++j) {
    s.cur = j & 1;
    split_seg_kernel<1><<<seg_grid, LANES, 0, st>>>(s);
    LAUNCH_CHECK();
  }
  s.cur = rounds & 1;
  split_verify_kernel<<<run_grid, LANES, 0, st>>>(s);
  LAUNCH_CHECK();
  split_seg_kernel<2><<<seg_grid, LANES, 0, st>>>(s);
  LAUNCH_CHECK();
  // what is left: the runs that were not split, and every run of an image whose split did not pass (path 2)
  Args a;
  a.p = *plan;
  a.g = s.g;
  a.status = status;
  a.info = s.s.info;
  a.path = path;
  a.lanes = lanes_per_wave(plan->nruns);
  decode_kernel<<<grid(cdiv(plan->nruns, a.lanes)), LANES, 0, st>>>(a);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

size_t rgbnm_jpeg_split_crop_scratch_bytes(size_t stream_bytes, int nruns, int seg_bits) {
  return jpegsplit::crop_scratch_bytes(stream_bytes, nruns, seg_bits);
}

int rgbnm_jpeg_decode_batch_split_crop(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, const int32_t* boxes,
                                       const long long* y_off, const long long* c_off, int16_t* Ypacked, size_t y_elems, int16_t* Cpacked,
                                       size_t c_elems, int32_t* status, int32_t* path, uint32_t* walked, uint32_t* seg_live, void* scratch,
                                       size_t scratch_bytes, int seg_bits, int rounds, void* stream) {
  using namespace jpegdec;
  if (bad_call(plan, n, Hb, Wb, Hbc, Wbc, Ypacked, Cpacked, status)) return RGBNM_EINVAL;
  if (!boxes || !y_off || !c_off || y_elems == 0 || c_elems == 0) return RGBNM_EINVAL;
  if (((uintptr_t)boxes & 3) || ((uintptr_t)y_off & 7) || ((uintptr_t)c_off & 7) || ((uintptr_t)walked & 3) || ((uintptr_t)seg_live & 3))
    return RGBNM_EINVAL;
  if (!path || ((uintptr_t)path & 3) || rounds < 0 || rounds > jpegsplit::ROUNDS_MAX) return RGBNM_EINVAL;
  const size_t need = jpegsplit::crop_scratch_bytes(plan->stream_bytes, plan->nruns, seg_bits);   // 0: seg_bits out of range
  if (need == 0 || !scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need) return RGBNM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  XArgs x;
  SArgs& s = x.s;
  s.p = *plan;
  s.g = out_of(n, Hb, Wb, Hbc, Wbc, nullptr, nullptr);
  s.path = path;
  s.s = jpegsplit::carve(scratch, plan->stream_bytes, plan->nruns, seg_bits);
  s.seg_bits = seg_bits;
  const int ms = rgbnm_get_option("jpeg_min_seg");
  s.min_seg = ms >= 2 ? ms : jpegsplit::MIN_SEG;
  s.cur = 0;
  s.lanes = 1;
  x.boxes = boxes; x.y_off = y_off; x.c_off = c_off;
  x.Y = Ypacked; x.C = Cpacked; x.y_elems = y_elems; x.c_elems = c_elems;
  x.status = status;
  x.walked = walked;
  x.seg_live = seg_live;
  x.x = jpegsplit::carve_crop(scratch, plan->stream_bytes, plan->nruns, seg_bits);
  x.run_lanes = 1;
  const int lanes_opt = rgbnm_get_option("jpeg_lanes");
  x.fixed_lanes = lanes_opt >= 1 && lanes_opt <= LANES;
  const int cap_opt = rgbnm_get_option("jpeg_split_wgs");          // as in the split call
  const int cap = cap_opt >= 1 && cap_opt < MAX_WGS ? cap_opt : MAX_WGS;
  auto grid = [cap](long long groups) { return (unsigned)(groups < 1 ? 1 : groups < cap ? groups : cap); };
  const long long nslots = s.s.nslots;
  split_crop_init_kernel<<<grid(cdivl(nslots > n ? nslots : n, 256)), 256, 0, st>>>(x);
  LAUNCH_CHECK();
  if (plan->nruns == 0) return RGBNM_OK;
  s.lanes = lanes_per_wave(nslots);
  x.run_lanes = lanes_per_wave(plan->nruns);
  const unsigned seg_grid = grid(cdivl(nslots, s.lanes)), run_grid = grid(plan->nruns);
  split_map_kernel<<<run_grid, LANES, 0, st>>>(s);
  LAUNCH_CHECK();
  split_seg_kernel<0><<<seg_grid, LANES, 0, st>>>(s);
  LAUNCH_CHECK();
  for (int j = 0; j < rounds; ++j) {
    s.cur = j & 1;
    split_seg_kernel<1><<<seg_grid, LANES, 0, st>>>(s);
    LAUNCH_CHECK();
  }
  s.cur = rounds & 1;
  split_verify_crop_kernel<<<run_grid, LANES, 0, st>>>(x);
  LAUNCH_CHECK();
  // over the list: its length is device data, so the grid is the whole-grid write pass's (enough for the list at any number of
  // entries per wave that the kernel's rule can choose, the grid-stride loop aside) and the waves behind the list's end leave at once
  split_write_crop_kernel<<<seg_grid, LANES, 0, st>>>(x);
  LAUNCH_CHECK();
  decode_crop_rest_kernel<<<grid(cdiv(plan->nruns, x.run_lanes)), LANES, 0, st>>>(x);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

}  // extern "C"
