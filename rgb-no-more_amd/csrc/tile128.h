// The [token][64] bf16 LDS arrays with 128-byte rows (chunk q of row r at q ^ fswz(r)) of attention_v2.hip, vit_chain.hip and
// vit_chain_bwd.hip: lane geometry, row and transposed MFMA fragments, and the gradient tiles the attention backward parks in LDS.
// ROWB is this family's pitch: files with another row pitch (gemm_nt_wres.hip: 384 bytes) include lds_common.h only.
#pragma once
#include <type_traits>
#include "lds_common.h"

namespace {

constexpr int ROWB = 128;                 // bytes per token row

struct Geo {
  int lane, l31, g, fl;
  unsigned tr0;    // byte offset inside a [token][64] array of the (t=0, fi=0, dt=0, rd=0) transpose read (tfrag4)
};
__device__ __forceinline__ Geo make_geo() {
  Geo L;
  L.lane = threadIdx.x & 63;
  L.l31 = L.lane & 31;
  L.g = L.lane >> 5;
  L.fl = fswz(L.l31);
  const int k = (L.lane >> 2) & 3, G1 = (L.lane >> 4) & 1, l3 = L.lane & 3;
  const int pc = (2 * G1 + (l3 >> 1)) ^ (((k >> 1) << 2) | L.g);
  L.tr0 = (unsigned)((4 * L.g + k) * ROWB + pc * 16 + 8 * (l3 & 1));
  return L;
}
// The same from a lane id the optimiser cannot trace (common.h lane_id_here): every phase derives its per-lane constants anew, so
// none of them is live -- or spilled -- across the register-heavy phases in between
__device__ __forceinline__ Geo fresh_geo() {
  Geo L;
  L.lane = lane_id_here();
  L.l31 = L.lane & 31;
  L.g = L.lane >> 5;
  L.fl = fswz(L.l31);
  const int k = (L.lane >> 2) & 3, G1 = (L.lane >> 4) & 1, l3 = L.lane & 3;
  const int pc = (2 * G1 + (l3 >> 1)) ^ (((k >> 1) << 2) | L.g);
  L.tr0 = (unsigned)((4 * L.g + k) * ROWB + pc * 16 + 8 * (l3 & 1));
  return L;
}

// f(0), f(1), ... f(T - 1) with the index as a compile-time constant (the tile number is an immediate offset of the transpose reads)
template <int T> struct TileLoop {
  template <typename F> static __device__ __forceinline__ void run(F&& f) {
    TileLoop<T - 1>::run(f);
    f(std::integral_constant<int, T - 1>{});
  }
};
template <> struct TileLoop<0> {
  template <typename F> static __device__ __forceinline__ void run(F&&) {}
};

// MFMA operand with the head dim as reduction axis (lane <-> token row 32 t + l31, 32-byte chunk c, half g), the per-lane part
// folded into one offset rb = l31 * ROWB + ((g ^ fswz(l31)) << 4): chunk c of the row is at rb ^ (c << 5) because
// (2c + g) ^ fl = 2c ^ (g ^ fl).  rb is re-derived (made opaque) at the start of each phase so the per-array, per-chunk addresses
// are not kept in registers -- or spilled -- across the whole persistent loop.
template <typename E = bf16>
__device__ __forceinline__ Frag<E> rowfrag_x(const unsigned char* arr, unsigned rb, int t, int c) {
  Frag<E> f;
  f.v = *reinterpret_cast<const typename Vec8<E>::type*>(arr + (rb ^ (unsigned)(c << 5)) + t * 32 * ROWB);
  return f;
}

// The eight MFMAs of one 32-row tile in the attention backward (scores and their gradient: two accumulators, K = 64 in four steps)
// with their eight row fragments in a PINNED order: four fragments ahead, every MFMA followed by the read of the fragment two steps
// on (into registers an earlier MFMA has read -- the sixteen the transposed fragments of the tile's second half take afterwards).
// Left alone the compiler emits read - wait - MFMA eight times with ONE fragment buffer: an exposed LDS latency per MFMA (50 of
// attn3_bwd's 196; 336 per block and wave of the chain backward).  Same MFMA order per accumulator as the plain loop: same bits.
template <typename E>
__device__ __forceinline__ void row_pair_mma(f32x16& sa, f32x16& da, const unsigned char* arrS, const unsigned char* arrD, unsigned rb,
                                             int t, const Frag<E> (&xs)[4], const Frag<E> (&xd)[4]) {
#define T128_SB __builtin_amdgcn_sched_barrier(0)
  Frag<E> fs[4], fd[4];
  T128_SB;
  fs[0] = rowfrag_x<E>(arrS, rb, t, 0);
  fd[0] = rowfrag_x<E>(arrD, rb, t, 0);
  fs[1] = rowfrag_x<E>(arrS, rb, t, 1);
  fd[1] = rowfrag_x<E>(arrD, rb, t, 1);
  T128_SB;
  mma(sa, fs[0], xs[0]); T128_SB;
  fs[2] = rowfrag_x<E>(arrS, rb, t, 2); T128_SB;
  mma(da, fd[0], xd[0]); T128_SB;
  fd[2] = rowfrag_x<E>(arrD, rb, t, 2); T128_SB;
  mma(sa, fs[1], xs[1]); T128_SB;
  fs[3] = rowfrag_x<E>(arrS, rb, t, 3); T128_SB;
  mma(da, fd[1], xd[1]); T128_SB;
  fd[3] = rowfrag_x<E>(arrD, rb, t, 3); T128_SB;
  mma(sa, fs[2], xs[2]);
  mma(da, fd[2], xd[2]);
  mma(sa, fs[3], xs[3]);
  mma(da, fd[3], xd[3]);
  T128_SB;
#undef T128_SB
}

// Transposed operands (tokens as reduction axis) of tile T of ONE array, both fragments (FI = 0, 1) x both 32-wide d tiles:
// 8 transpose reads, one wait.  a0 = array address + Geo::tr0, the per-lane address for (fi=0, dt=0, rd=0); dt=1 flips address
// bit 6, rd=1 flips bit 5 and adds 8 rows, fi=1 adds 16 rows.
template <int T, typename E>
__device__ __forceinline__ void tfrag4(unsigned a0, Frag<E> (&f)[4]) {
  u32x2 r0, r1, r2, r3, r4, r5, r6, r7;
  const unsigned a00 = a0, a01 = (a0 ^ 32u) + 1024u, a10 = a0 ^ 64u, a11 = (a0 ^ 96u) + 1024u;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8 offset:%12\n\t"
      "ds_read_b64_tr_b16 %1, %9 offset:%12\n\t"
      "ds_read_b64_tr_b16 %2, %10 offset:%12\n\t"
      "ds_read_b64_tr_b16 %3, %11 offset:%12\n\t"
      "ds_read_b64_tr_b16 %4, %8 offset:%13\n\t"
      "ds_read_b64_tr_b16 %5, %9 offset:%13\n\t"
      "ds_read_b64_tr_b16 %6, %10 offset:%13\n\t"
      "ds_read_b64_tr_b16 %7, %11 offset:%13\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)
      : "v"(a00), "v"(a01), "v"(a10), "v"(a11), "i"(T * 4096), "i"(T * 4096 + 2048)
      : "memory");
  __builtin_amdgcn_sched_barrier(0);
  f[0].v = pack8_as<E>(r0, r1);   // fi=0, dt=0
  f[1].v = pack8_as<E>(r2, r3);   // fi=0, dt=1
  f[2].v = pack8_as<E>(r4, r5);   // fi=1, dt=0
  f[3].v = pack8_as<E>(r6, r7);   // fi=1, dt=1
}
// The same through the compiler's builtin (lds_common.h tr_read): the reads can be requested ahead and waited for where they are
// used; the asm form above waits on the spot.  a0 = Geo::tr0 relative to smem
template <int T, typename E>
__device__ __forceinline__ void tfrag4_b(const unsigned char* smem, unsigned a0, Frag<E> (&f)[4]) {
  const unsigned a00 = a0, a01 = (a0 ^ 32u) + 1024u, a10 = a0 ^ 64u, a11 = (a0 ^ 96u) + 1024u;
  f[0].v = pack8_as<E>(tr_read(smem, a00 + T * 4096), tr_read(smem, a01 + T * 4096));
  f[1].v = pack8_as<E>(tr_read(smem, a10 + T * 4096), tr_read(smem, a11 + T * 4096));
  f[2].v = pack8_as<E>(tr_read(smem, a00 + T * 4096 + 2048), tr_read(smem, a01 + T * 4096 + 2048));
  f[3].v = pack8_as<E>(tr_read(smem, a10 + T * 4096 + 2048), tr_read(smem, a11 + T * 4096 + 2048));
}

// Between a wave's accesses to ITS OWN LDS tile (write the fragment layout, read row pieces back, overwrite with the next tile) no
// wait is needed: the LDS executes one wave's DS instructions in order, and the compiler counts lgkmcnt for the registers that are
// used.  What must not happen is the compiler reordering the accesses (differently typed pointers): a compiler-only fence.  The
// drains that stood here cost two LDS round trips per stored tile (~50 tiles per block and wave).
__device__ __forceinline__ void own_tile_fence() { asm volatile("" ::: "memory"); }

// LDS-DMA of one [N][64] bf16 matrix (row stride ld elements) into an array by ONE wave: 28 instructions of 1 KB (8 rows).
// Rows >= N replicate row N - 1 (finite data; their probabilities are masked to zero).
template <typename E>
__device__ __forceinline__ void dma_matrix_all(const E* __restrict__ src, int ld, int N, unsigned char* dst, int lane) {
#pragma unroll 4
  for (int i = 0; i < 28; ++i) {
    const int row = 8 * i + (lane >> 3), pc = lane & 7;
    const int lc = pc ^ fswz(row);
    const int srow = row < N ? row : N - 1;
    __builtin_amdgcn_global_load_lds((glb_ptr)(src + (size_t)srow * ld + lc * 8), (lds_ptr)(dst + i * 1024), 16, 0, 0);
  }
}

// ---- Gradient tiles of the attention backward.  Gradient rows leave it as full 128-byte lines, and not from the compute waves.
// In the swapped orientation a lane owns one token and 4 consecutive head-dim values per accumulator quad, so direct stores are
// 8 bytes per lane at a 1152-byte stride; worse, every CU reaches its store / load burst at the same time and a vmem instruction
// then takes ~700-1000 cycles to ISSUE (cycle stamps: 40 % of a pair's time went to issuing 24 stores, 13 loads and 16 LDS-DMAs
// per wave).  So the compute waves only park their 32 x 64 bf16 tiles in LDS (8-byte writes, conflict free):
//   dQ -> the wave's own rows of Ks (free after the mid barrier),  dK -> a private 4.5 KB tile,  dV -> own rows of Gs
// and the DMA wave reads them back as 16 B per lane, 8 lanes per row, and issues every global store (whole lines).
constexpr int STG_PITCH = 144;
constexpr int STG_WAVE = 32 * STG_PITCH;       // 4.5 KB per wave
template <typename E = bf16>
__device__ __forceinline__ void tile_park_private(unsigned char* stg, const f32x16 (&acc)[2], float mul, const Geo& L) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      f32x4 v = {acc[dt][rq * 4 + 0], acc[dt][rq * 4 + 1], acc[dt][rq * 4 + 2], acc[dt][rq * 4 + 3]};
      store4<E>(reinterpret_cast<E*>(stg + L.l31 * STG_PITCH) + dt * 32 + rq * 8 + L.g * 4, v * mul);
    }
}
// rows w*32 .. w*32+31 of a 128-byte-pitch array; 16-byte chunk c of row r sits at chunk c ^ (r & 7)
template <typename E = bf16>
__device__ __forceinline__ void tile_park_rows(unsigned char* arr, int w, const f32x16 (&acc)[2], float mul) {
  // one opaque base offset, chunk selected by XOR with a constant: the 8 swizzled addresses are loop invariants that the
  // compiler otherwise hoists to the kernel prologue and then SPILLS (each reload a serialised scratch round trip)
  const int ln = lane_id_here();   // (and off0 itself is recomputed here, not kept live across the pair)
  const unsigned off0 = (unsigned)((w * 32 + (ln & 31)) * ROWB + ((ln & 7) << 4) + (ln >> 5) * 8);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      f32x4 v = {acc[dt][rq * 4 + 0], acc[dt][rq * 4 + 1], acc[dt][rq * 4 + 2], acc[dt][rq * 4 + 3]};
      store4<E>(reinterpret_cast<E*>(arr + (off0 ^ (unsigned)((dt * 4 + rq) << 4))), v * mul);
    }
}
// DMA wave: the parked tiles of the NT compute waves whose rows start below N (private tiles, or rows of an array) -> registers;
// the files' own tiles_write sends them on to global rows
template <bool PRIVATE, int NT>
__device__ __forceinline__ void tiles_read(const unsigned char* src, int N, int lane, u32x4 (&v)[NT][4]) {
  const int rl = lane >> 3, seg = lane & 7;
#pragma unroll
  for (int wv = 0; wv < NT; ++wv) {
    if (wv * 32 < N) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = i * 8 + rl;
        v[wv][i] = PRIVATE ? *reinterpret_cast<const u32x4*>(src + wv * STG_WAVE + r * STG_PITCH + seg * 16)
                           : *reinterpret_cast<const u32x4*>(src + (wv * 32 + r) * ROWB + ((seg ^ (r & 7)) << 4));
      }
    }
  }
}

}  // namespace
