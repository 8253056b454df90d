// Entropy ENCODING of baseline JPEG files on the device (include/rgbnm.h: rgbnm_jpeg_encode_batch): from the int16 coefficient
// tensors of the decode to whole files, SOI to EOI, byte for byte what libjpeg's jpeg_write_coefficients writes with its defaults
// (T.81 Annex K tables, 4:2:0 or one component), optionally with restart markers.  The per-block logic is jpeg_emit.h, shared with
// the stand-alone host check; this file is the four launches around it.  Every image of a batch has the same block grids, so block b
// of image i is the same place of the scan in every image and all work is indexed, never walked:
//
//   1 measure  one lane per block of the MCU-padded scan order: DC difference (predecessor found by index), bit length of the block
//              (LEN_ERANGE where a value does not fit baseline coding) -> pos[]; the same launch zeroes the raw streams
//   2 place    one workgroup per image: a prefix scan over the image's blocks, 256 per trip, of the functions "add the length" /
//              "go to the next byte, then add" (first block of a restart run) turns pos[] into bit positions in the image's raw stream
//              and gives run_start[]; checks dims and quant; writes the image's record (status, raw bytes)
//   3 emit     one lane per block again: codes the block a second time, now into its position.  Whole words are stored; the first
//              and last word of a block are shared with its neighbours and merged by integer atomic OR into the zeroed stream
//              (associative and commutative: the bytes do not depend on the order of arrival).  The last block of a run pads with 1s.
//   4 stuff    one workgroup per image: counts the FF bytes, refuses the image if the file would not fit, writes the header, then
//              moves the raw bytes 16 per lane to header + i + (FFs before) + 2 * run, adding 00 behind FF and RSTn between runs, EOI
//
// The raw stream of an image lives in scratch with room for `stride` bytes (a file never is shorter than its raw stream), so a failed
// image (range, capacity, dims) leaves its slot of `out` untouched.  All loops are bounded by the grid constants or by counts the
// kernels computed and checked against the buffers; every store is checked against its buffer.
#include "common.h"
#include "jpeg_emit.h"
#include "../../include/rgbnm.h"

namespace jpegenc {

using namespace jpegemit;

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int MAX_WGS = 4096;
static_assert(ST_EGRID == RGBNM_JPEG_EGRID && ST_ECAPACITY == RGBNM_JPEG_ECAPACITY && ST_ERANGE == RGBNM_JPEG_ERANGE, "status codes");

__device__ const Std d_std = JPEGEMIT_STD_INIT;
constexpr Std h_std = JPEGEMIT_STD_INIT;
__device__ const Codes d_codes = make_codes(h_std);

// The scratch of one call, carved the same way by the size function and the launch
struct Scratch {
  uint32_t* pos;                           // [n][nblocks]   bit length, then bit position in the image's raw stream
  uint32_t* run_start;                     // [n][nruns + 1] raw byte at which each run begins; the last entry is the raw size
  int32_t* rec;                            // [n][2]         status, raw bytes
  uint8_t* raw;                            // [n][rawcap]    un-stuffed scan bytes, zero beyond the raw size
  uint32_t rawcap;                         // multiple of 16; at least 16 more than any raw stream that is emitted
  size_t bytes;
};
__host__ inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
__host__ Scratch carve(void* base, int n, const Geo& g, size_t stride) {
  Scratch s;
  const size_t bound = file_bound(g);
  const size_t cap = up16(stride < bound ? stride : bound) + 16;       // < 2^32: make_geo bounds the bits of an image
  uint8_t* p = (uint8_t*)base;
  size_t off = 0;
  s.pos = (uint32_t*)(p + off); off += up16((size_t)n * g.nblocks * 4);
  s.run_start = (uint32_t*)(p + off); off += up16((size_t)n * (g.nruns + 1) * 4);
  s.rec = (int32_t*)(p + off); off += up16((size_t)n * 8);
  s.raw = p + off; off += (size_t)n * cap;
  s.rawcap = (uint32_t)cap;
  s.bytes = off;
  return s;
}

struct Args {
  Geo g;
  Scratch s;
  int n;
  const int16_t* Y;
  const int16_t* C;
  const int16_t* quant;                    // [n][ncomp][64]
  const int32_t* dims;                     // [n][2] height, width
  uint8_t* out;
  size_t stride;
  int32_t* nbytes;
  int32_t* status;
};

struct CoefDC {                            // DC of a real block
  const Args& a;
  int img;
  __device__ int operator()(int comp, int by, int bx) const { return (comp ? a.C : a.Y)[coef_offset(a.g, img, comp, by, bx)]; }
};
struct CoefAC {                            // the block's 64 coefficients in registers; indices are constants after unrolling
  uint32_t w[32];
  __device__ int operator()(int i) const { return (int)(int16_t)(w[i >> 1] >> ((i & 1) * 16)); }
};
__device__ inline void load_block(CoefAC& c, const int16_t* p) {
  const uint4* q = (const uint4*)p;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint4 v = q[k];
    c.w[4 * k] = v.x; c.w[4 * k + 1] = v.y; c.w[4 * k + 2] = v.z; c.w[4 * k + 3] = v.w;
  }
}
__device__ inline void stage_codes(Codes& sh) {
  const uint32_t* src = (const uint32_t*)&d_codes;
  uint32_t* dst = (uint32_t*)&sh;
  for (int i = threadIdx.x; i < (int)(sizeof(Codes) / 4); i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}

// ---- 1 measure ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void measure_kernel(Args a) {
  __shared__ Codes codes;
  stage_codes(codes);
  const size_t tid = (size_t)blockIdx.x * THREADS + threadIdx.x, nthreads = (size_t)gridDim.x * THREADS;
  const size_t nz = (size_t)a.n * a.s.rawcap / 16;
  for (size_t i = tid; i < nz; i += nthreads) ((uint4*)a.s.raw)[i] = make_uint4(0, 0, 0, 0);
  const size_t total = (size_t)a.n * a.g.nblocks;
  for (size_t idx = tid; idx < total; idx += nthreads) {
    const int img = (int)(idx / a.g.nblocks), b = (int)(idx - (size_t)img * a.g.nblocks);
    const Blk k = block_at(a.g, b);
    const int diff = dc_diff(a.g, k, CoefDC{a, img});
    CoefAC c;
    if (k.real) load_block(c, (k.comp ? a.C : a.Y) + coef_offset(a.g, img, k.comp, k.by, k.bx));
    BitCount cnt;
    const bool ok = code_block(codes, k.comp ? 1 : 0, diff, k.real, c, cnt);
    a.s.pos[idx] = ok ? cnt.bits : LEN_ERANGE;
  }
}

// ---- 2 place ------------------------------------------------------------------------------------------------------------------------
__device__ inline Fn shfl_up_fn(const Fn& v, int d) {
  return Fn{(uint32_t)__shfl_up((int)v.a, d, WAVE), (uint32_t)__shfl_up((int)v.s, d, WAVE), (uint32_t)__shfl_up((int)v.f, d, WAVE)};
}
__global__ __launch_bounds__(THREADS) void place_kernel(Args a) {
  __shared__ Fn wave_tot[THREADS / WAVE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const Geo& g = a.g;
  const int per_run = g.ri * g.nblk;
  for (int img = blockIdx.x; img < a.n; img += gridDim.x) {
    // what the image's own arguments say
    int st = 0;
    if (tid == 0 && !dims_fit(g, a.dims[2 * img], a.dims[2 * img + 1])) st = ST_EGRID;
    int qbad = 0;
    for (int i = tid; i < (g.ncomp == 3 ? 128 : 64); i += THREADS) {
      const int q = a.quant[(size_t)img * g.ncomp * 64 + i];
      qbad |= q < 1 || q > 255;
    }
    uint32_t carry = 0;
    int bad = 0;
    for (int base = 0; base < g.nblocks; base += THREADS) {
      const int b = base + tid;
      uint32_t len = b < g.nblocks ? a.s.pos[(size_t)img * g.nblocks + b] : 0;
      if (len == LEN_ERANGE) { bad = 1; len = 0; }
      const bool first = b < g.nblocks && b % per_run == 0;
      Fn f{0, len, first ? 1u : 0u};
      for (int d = 1; d < WAVE; d <<= 1) {             // inclusive scan in the wave
        const Fn up = shfl_up_fn(f, d);
        if (lane >= d) f = compose(up, f);
      }
      __syncthreads();                                 // wave_tot of the trip before has been read
      if (lane == WAVE - 1) wave_tot[wave] = f;
      __syncthreads();
      Fn before{0, 0, 0};                              // the waves before this one
      for (int w = 0; w < wave; ++w) before = compose(before, wave_tot[w]);
      Fn all = before;
      for (int w = wave; w < THREADS / WAVE; ++w) all = compose(all, wave_tot[w]);
      const uint32_t end = apply(compose(before, f), carry);
      if (b < g.nblocks) {
        a.s.pos[(size_t)img * g.nblocks + b] = end - len;
        if (first) a.s.run_start[(size_t)img * (g.nruns + 1) + b / per_run] = (end - len) >> 3;
      }
      carry = apply(all, carry);
    }
    bad = __syncthreads_or(bad | qbad);
    st = __syncthreads_or(st != 0) ? ST_EGRID : 0;
    if (tid == 0) {
      const uint32_t rawbytes = align8(carry) >> 3;
      if (st == 0 && bad) st = ST_ERANGE;
      if (st == 0 && ((size_t)rawbytes + 16 > a.s.rawcap || (size_t)file_size(g, rawbytes, 0) > a.stride)) st = ST_ECAPACITY;
      a.s.rec[2 * img] = st;
      a.s.rec[2 * img + 1] = (int32_t)rawbytes;
      a.s.run_start[(size_t)img * (g.nruns + 1) + g.nruns] = rawbytes;
    }
  }
}

// ---- 3 emit -------------------------------------------------------------------------------------------------------------------------
struct RawMem {                            // an image's raw stream as big-endian words
  uint32_t* words;
  uint32_t nwords;
  __device__ void set_word(uint32_t i, uint32_t v) { if (i < nwords) words[i] = __builtin_bswap32(v); }
  __device__ void or_word(uint32_t i, uint32_t v) { if (i < nwords && v) atomicOr(&words[i], __builtin_bswap32(v)); }
};
__global__ __launch_bounds__(THREADS) void emit_kernel(Args a) {
  __shared__ Codes codes;
  stage_codes(codes);
  const size_t tid = (size_t)blockIdx.x * THREADS + threadIdx.x, nthreads = (size_t)gridDim.x * THREADS;
  const size_t total = (size_t)a.n * a.g.nblocks;
  const int per_run = a.g.ri * a.g.nblk;
  for (size_t idx = tid; idx < total; idx += nthreads) {
    const int img = (int)(idx / a.g.nblocks), b = (int)(idx - (size_t)img * a.g.nblocks);
    if (a.s.rec[2 * img] != 0) continue;
    const Blk k = block_at(a.g, b);
    const int diff = dc_diff(a.g, k, CoefDC{a, img});
    CoefAC c;
    if (k.real) load_block(c, (k.comp ? a.C : a.Y) + coef_offset(a.g, img, k.comp, k.by, k.bx));
    RawMem mem{(uint32_t*)(a.s.raw + (size_t)img * a.s.rawcap), a.s.rawcap / 4};
    BitSink<RawMem> sink(mem, a.s.pos[idx]);
    code_block(codes, k.comp ? 1 : 0, diff, k.real, c, sink);
    if ((b + 1) % per_run == 0 || b + 1 == a.g.nblocks) sink.pad_to_byte();
    sink.flush();
  }
}

// ---- 4 stuff ------------------------------------------------------------------------------------------------------------------------
struct OutBytes {
  uint8_t* p;
  size_t cap;
  __device__ void put(uint32_t pos, uint8_t v) { if (pos < cap) p[pos] = v; }
};
// Inclusive sum over the workgroup; *total: the sum of all.  Two barriers; `sh` is free again after the second.
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  for (int d = 1; d < WAVE; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)v, d, WAVE);
    if (lane >= d) v += up;
  }
  __syncthreads();
  if (lane == WAVE - 1) sh[wave] = v;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int w = 0; w < THREADS / WAVE; ++w) {
    if (w < wave) before += sh[w];
    all += sh[w];
  }
  *total = all;
  return v + before;
}
__global__ __launch_bounds__(THREADS) void stuff_kernel(Args a) {
  __shared__ uint32_t sh[THREADS / WAVE];
  const int tid = threadIdx.x;
  const Geo& g = a.g;
  const uint32_t hdr = (uint32_t)header_bytes(g);
  constexpr uint32_t TRIP = THREADS * 16;
  for (int img = blockIdx.x; img < a.n; img += gridDim.x) {
    int st = a.s.rec[2 * img];
    const uint32_t rawbytes = (uint32_t)a.s.rec[2 * img + 1];
    const uint8_t* raw = a.s.raw + (size_t)img * a.s.rawcap;
    if (st != 0 || (size_t)rawbytes + 16 > a.s.rawcap) {         // the second never holds for a record with status 0
      if (tid == 0) { a.status[img] = st ? st : ST_ECAPACITY; a.nbytes[img] = 0; }
      continue;
    }
    uint32_t mine = 0, nff = 0;
    for (uint32_t i = (uint32_t)tid * 16; i < rawbytes; i += TRIP) {
      const uint4 v = *(const uint4*)(raw + i);                  // bytes beyond rawbytes are zero
      mine += count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);
    }
    block_scan(mine, sh, &nff);
    const size_t size = file_size(g, rawbytes, nff);
    if (size > a.stride) {
      if (tid == 0) { a.status[img] = ST_ECAPACITY; a.nbytes[img] = 0; }
      continue;
    }
    OutBytes out{a.out + (size_t)img * a.stride, a.stride};
    const int32_t* dim = a.dims + 2 * img;
    for (uint32_t i = tid; i < hdr; i += THREADS)
      out.put(i, header_byte(d_std, g, (int)i, dim[0], dim[1], a.quant + (size_t)img * g.ncomp * 64));
    const uint32_t* run_start = a.s.run_start + (size_t)img * (g.nruns + 1);
    uint32_t carry = 0;
    for (uint32_t base = 0; base < rawbytes; base += TRIP) {
      const uint32_t i0 = base + (uint32_t)tid * 16, i1 = i0 + 16 < rawbytes ? i0 + 16 : rawbytes;
      uint32_t c = 0, all;
      if (i0 < rawbytes) {
        const uint4 v = *(const uint4*)(raw + i0);
        c = count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);
      }
      const uint32_t incl = block_scan(c, sh, &all);
      stuff_chunk(raw, i0, i1, run_start, g.nruns, carry + incl - c, hdr, out);
      carry += all;
    }
    if (tid == 0) {
      out.put((uint32_t)size - 2, 0xFF);
      out.put((uint32_t)size - 1, 0xD9);
      a.status[img] = 0;
      a.nbytes[img] = (int32_t)size;
    }
  }
}

}  // namespace jpegenc

extern "C" {

size_t rgbnm_jpeg_encode_bound(int Hb, int Wb, int Hbc, int Wbc, int ncomp, int restart) {
  jpegemit::Geo g;
  return jpegemit::make_geo(g, Hb, Wb, Hbc, Wbc, ncomp, restart) ? jpegemit::file_bound(g) : 0;
}

size_t rgbnm_jpeg_encode_scratch_bytes(int n, int Hb, int Wb, int Hbc, int Wbc, int ncomp, int restart, size_t stride) {
  jpegemit::Geo g;
  if (n <= 0 || stride == 0 || !jpegemit::make_geo(g, Hb, Wb, Hbc, Wbc, ncomp, restart)) return 0;
  return jpegenc::carve(nullptr, n, g, stride).bytes;
}

int rgbnm_jpeg_encode_header(int ncomp, int height, int width, const int16_t* quant, int restart, uint8_t* out, size_t cap) {
  using namespace jpegemit;
  Geo g;
  if (!quant || !out || height < 1 || width < 1 || height > 65535 || width > 65535) return RGBNM_EINVAL;
  if (!make_geo(g, cdiv(height, 8), cdiv(width, 8), cdiv(height, 16), cdiv(width, 16), ncomp, restart)) return RGBNM_EINVAL;
  for (int i = 0; i < (ncomp == 3 ? 128 : 64); ++i)
    if (quant[i] < 1 || quant[i] > 255) return RGBNM_EINVAL;
  const int len = header_bytes(g);
  if ((size_t)len > cap) return RGBNM_EINVAL;
  for (int i = 0; i < len; ++i) out[i] = header_byte(jpegenc::h_std, g, i, height, width, quant);
  return len;
}

int rgbnm_jpeg_encode_batch(const int16_t* Y, const int16_t* CbCr, const int16_t* quant, const int32_t* dims, int n, int Hb, int Wb,
                            int Hbc, int Wbc, int restart, uint8_t* out, size_t stride, int32_t* nbytes, int32_t* status,
                            void* scratch, size_t scratch_bytes, void* stream) {
  using namespace jpegenc;
  Args a;
  if (!Y || !quant || !dims || !out || !nbytes || !status || !scratch || n <= 0 || stride == 0 || stride >= ((size_t)1 << 31))
    return RGBNM_EINVAL;
  if (!make_geo(a.g, Hb, Wb, Hbc, Wbc, CbCr ? 3 : 1, restart)) return RGBNM_EINVAL;
  if (((uintptr_t)Y & 15) || ((uintptr_t)CbCr & 15) || ((uintptr_t)quant & 1) || ((uintptr_t)dims & 3) || ((uintptr_t)nbytes & 3) ||
      ((uintptr_t)status & 3) || ((uintptr_t)scratch & 15))
    return RGBNM_EINVAL;
  if ((size_t)n * a.g.nblocks >= ((size_t)1 << 40)) return RGBNM_EINVAL;
  a.s = carve(scratch, n, a.g, stride);
  if (scratch_bytes < a.s.bytes) return RGBNM_EINVAL;
  a.n = n; a.Y = Y; a.C = CbCr; a.quant = quant; a.dims = dims; a.out = out; a.stride = stride; a.nbytes = nbytes; a.status = status;
  // Option "jpeg_encode_wgs" caps the workgroups of every launch (tests: each grid-stride loop goes round again).
  const int cap_opt = rgbnm_get_option("jpeg_encode_wgs");
  const long long cap = cap_opt >= 1 && cap_opt < MAX_WGS ? cap_opt : MAX_WGS;
  const long long per_block = ((long long)n * a.g.nblocks + THREADS - 1) / THREADS;
  const unsigned block_grid = (unsigned)(per_block < cap ? per_block : cap), image_grid = (unsigned)(n < cap ? n : cap);
  hipStream_t st = (hipStream_t)stream;
  measure_kernel<<<block_grid, THREADS, 0, st>>>(a);
  LAUNCH_CHECK();
  place_kernel<<<image_grid, THREADS, 0, st>>>(a);
  LAUNCH_CHECK();
  emit_kernel<<<block_grid, THREADS, 0, st>>>(a);
  LAUNCH_CHECK();
  stuff_kernel<<<image_grid, THREADS, 0, st>>>(a);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

}  // extern "C"
