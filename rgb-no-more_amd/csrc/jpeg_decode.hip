// Entropy decoding of baseline JPEG files on the device (include/rgbnm.h: rgbnm_jpeg_prepare, rgbnm_jpeg_decode_batch).
//
// The host finds the independent bit streams ("runs": the scan, or one per restart interval) -- jpeg_scan.h, a byte scan -- and the
// kernel below walks them, ONE LANE PER RUN, grid-strided over the run records (1 to 64 runs per wave, see the launch).  The walk
// itself is jpeg_walk.h, shared with the stand-alone host check.  What this file adds is the wave's side of it:
//   - workgroup = one wave of 64 lanes; each lane owns a 128-byte block tile in LDS (pitch 144 bytes, so that the 16-byte moves stay
//     aligned and neighbouring lanes start 36 banks apart).  The walk scatters 2-byte coefficients into the tile; a finished block
//     leaves as eight 16-byte stores -- whole 128-byte lines, zeros included, so no fill launch precedes the kernel -- and the tile
//     is zeroed by the same pass.
//   - the Huffman tables (1440 bytes each in look-up form) are staged in LDS when every live lane of the wave uses the same six
//     (DC / AC per component), which is the common case: a dataset written by one encoder carries the four standard tables in every
//     file.  Otherwise the lanes read the batch's table array in global memory.  The choice is wave-uniform.
//   - an error lowers status[image] with atomicMin; no lane waits for another, no loop depends on the data for its bound.
#include "common.h"
#include "jpeg_scan.h"
#include "jpeg_walk.h"
#include "../../include/rgbnm.h"

namespace jpegdec {

constexpr int LANES = 64;
constexpr int PITCH = 144;                 // bytes between the tiles of neighbouring lanes
constexpr int SLOTS = 6;                   // staged tables: slot 2 c = DC of component c, 2 c + 1 = AC
constexpr int MAX_WGS = 4096;
constexpr int TAB_PIECES = (int)(sizeof(rgbnm_jpeg_hufftab) / 16);

__device__ const uint8_t d_zigzag[64] = {JPEGSCAN_ZIGZAG_VALUES};

struct Args {
  rgbnm_jpeg_device_plan p;
  jpegwalk::Out g;
  int32_t* status;
  int lanes;                               // runs per wave, 1..64
};

__global__ __launch_bounds__(LANES) void decode_kernel(Args a) {
  using namespace jpegwalk;
  __shared__ alignas(16) uint8_t s_tile[LANES * PITCH];
  __shared__ alignas(16) rgbnm_jpeg_hufftab s_tab[SLOTS];
  __shared__ uint8_t s_zz[64];
  const int lane = threadIdx.x;
  int16_t* tile = reinterpret_cast<int16_t*>(s_tile + lane * PITCH);
  s_zz[lane] = d_zigzag[lane];
  {
    V16* t = reinterpret_cast<V16*>(tile);
    const V16 zero = {0, 0, 0, 0};
    for (int j = 0; j < 8; ++j) t[j] = zero;
  }
  __syncthreads();
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
      }
    }
    // one table set for the whole wave?
    const unsigned long long mask = __ballot(live);
    if (mask == 0) continue;
    const int first = __ffsll((long long)mask) - 1;
    const uint64_t dc0 = __shfl((unsigned long long)L.dcsel, first, LANES), ac0 = __shfl((unsigned long long)L.acsel, first, LANES);
    const bool shared = __all(!live || (L.dcsel == dc0 && L.acsel == ac0));
    int err = 0;
    if (shared) {
      __syncthreads();                     // the previous round's readers of s_tab are done
      for (int j = lane; j < SLOTS * TAB_PIECES; j += LANES) {
        const int slot = j / TAB_PIECES, piece = j - slot * TAB_PIECES;
        const uint32_t t = (uint32_t)(((slot & 1) ? ac0 : dc0) >> (16 * (slot >> 1))) & 0xFFFFu;   // < ntables: check_run
        reinterpret_cast<V16*>(&s_tab[slot])[piece] = reinterpret_cast<const V16*>(&a.p.tables[t])[piece];
      }
      __syncthreads();
      if (live) {
        Lane S = L;
        S.dcsel = 0ull | (2ull << 16) | (4ull << 32);
        S.acsel = 1ull | (3ull << 16) | (5ull << 32);
        err = decode_run(a.p.stream, r, S, s_tab, s_zz, a.g, tile);
      }
    } else if (live) {
      err = decode_run(a.p.stream, r, L, a.p.tables, s_zz, a.g, tile);
    }
    if (live) {
      if (err) atomicMin(&a.status[r.image], err);
      if (L.ncomp == 1) zero_chroma_share(a.g, r.image, (uint32_t)r.mcu0, (uint32_t)r.nmcu, L.total);
    }
  }
}

}  // namespace jpegdec

extern "C" {

int rgbnm_jpeg_prepare(const uint8_t* const* bufs, const size_t* lens, int n, int Hb, int Wb, int Hbc, int Wbc, rgbnm_jpeg_plan* plan) {
  return jpegscan::prepare(bufs, lens, n, Hb, Wb, Hbc, Wbc, plan);
}

int rgbnm_jpeg_decode_batch(const rgbnm_jpeg_device_plan* plan, int n, int Hb, int Wb, int Hbc, int Wbc, int16_t* Y, int16_t* CbCr,
                            int32_t* status, void* stream) {
  using namespace jpegdec;
  if (!plan || !Y || !CbCr || !status || n <= 0 || Hb < 1 || Wb < 1 || Hbc < 1 || Wbc < 1 || Hb > 4096 || Wb > 4096 || Hbc > 4096 ||
      Wbc > 4096 || plan->nruns < 0 || plan->ntables < 0)
    return RGBNM_EINVAL;
  if (((uintptr_t)Y & 15) || ((uintptr_t)CbCr & 15) || ((uintptr_t)status & 3)) return RGBNM_EINVAL;
  if (plan->nruns == 0) return RGBNM_OK;
  if (!plan->stream || !plan->runs || !plan->images || !plan->tables || ((uintptr_t)plan->stream & 3) || ((uintptr_t)plan->tables & 15) ||
      ((uintptr_t)plan->runs & 3) || ((uintptr_t)plan->images & 3))
    return RGBNM_EINVAL;
  Args a;
  a.p = *plan;
  a.g.n = n; a.g.Hb = Hb; a.g.Wb = Wb; a.g.Hbc = Hbc; a.g.Wbc = Wbc; a.g.Y = Y; a.g.C = CbCr;
  a.status = status;
  // Runs per wave.  What is rare for a lane -- a code longer than 9 bits, a refill, the end of a block -- happens in almost every
  // trip of a wave whose 64 lanes all walk, and the wave pays for each.  A batch rarely has runs for every SIMD of the device
  // (256 without restart markers, 8192 with one per MCU row), so the runs are spread over about 2048 waves first and the waves fill
  // up only beyond that.  Option "jpeg_lanes" (1..64) fixes the number instead.
  const int opt = rgbnm_get_option("jpeg_lanes");
  int per = opt >= 1 && opt <= LANES ? opt : cdiv(plan->nruns, 2048);
  per = per < 1 ? 1 : per > LANES ? LANES : per;
  a.lanes = per;
  const int groups = cdiv(plan->nruns, per);
  decode_kernel<<<groups < MAX_WGS ? groups : MAX_WGS, LANES, 0, (hipStream_t)stream>>>(a);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

}  // extern "C"
