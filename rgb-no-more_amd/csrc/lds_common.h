// LDS conventions shared by the bf16 kernels, the part that knows no tile geometry: address-space and vector types, the chunk
// swizzle, packing, transpose reads, waits, barriers and the linear LDS-DMA.  One definition each: the swizzle and the packed
// layouts are a contract BETWEEN files (the chain kernels read weight images written "exactly as they lie in LDS", the backward
// reads what the forward's conventions stored), so a change here changes every user at once.  The [token][64] family with
// 128-byte rows is in tile128.h.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* glb_ptr;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef bf16 bf16x4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4v* lds_b64_ptr;

// One XOR swizzle of the 16-byte chunk index inside each 128 bytes of a row, f(row) = rot3((row >> 1) & 7): chunk q of `row` lies
// at q ^ fswz(row).  It makes BOTH access patterns bank-conflict free: ds_read_b128 of 32 token rows and ds_read_b64_tr_b16 of
// 4 rows x 64 B.  The chain kernels' weight images are laid out on the host with the same function: chain.py::_fswz, whose index
// tables rgbnm_chain_gather (vit_chain.hip) applies, MUST agree with this one.
__device__ __forceinline__ int fswz(int row) {
  return (((row >> 1) & 1) << 2) | ((row >> 2) & 1) | (((row >> 3) & 1) << 1);
}
// rows longer than 128 bytes: physical 16-byte chunk of logical chunk lc in `row` (an involution; the swizzle stays inside each 128 bytes)
__device__ __forceinline__ int pchunk(int lc, int row) { return (lc & ~7) | ((lc & 7) ^ fswz(row)); }

__device__ __forceinline__ unsigned pack2(float a, float b) {       // two fp32 -> bf16 pair (round to nearest even), a in the low half
  const bf16x2v v = {(bf16)a, (bf16)b};
  unsigned r = __builtin_bit_cast(unsigned, v);
  asm volatile("" : "+v"(r));     // packed HERE: the optimiser otherwise sinks the conversion to the (conditional) use and keeps the fp32 pair
  return r;
}
__device__ __forceinline__ bf16x8 pack8(u32x2 lo, u32x2 hi) {
  u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(bf16x8, v);
}
template <typename E> __device__ __forceinline__ typename Vec8<E>::type pack8_as(u32x2 lo, u32x2 hi) {   // the same bits as 8 x E
  u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(typename Vec8<E>::type, v);
}
__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

// ds_read_b64_tr_b16 through the compiler's builtin: an ordinary DS load to the scheduler (it can be requested ahead and waited
// for where it is used; the asm forms of the kernel files wait on the spot)
__device__ __forceinline__ u32x2 tr_read(const unsigned char* smem, unsigned off) {
  return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b64_ptr)(smem + off)));
}

// A per-lane value the optimiser must treat as new: addresses derived from it are re-derived where they are used (one XOR / add
// each) instead of being hoisted out of the block loop as invariants and spilled (common.h, lane_id_here)
__device__ __forceinline__ unsigned opaque(unsigned v) {
  asm volatile("" : "+v"(v));
  return v;
}
// workgroup barrier that the compiler may not move LDS / global accesses across (the builtin alone is "no memory")
__device__ __forceinline__ void wg_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// LDS-DMA of NKB linear 1 KB pieces by one wave (16 B per lane)
template <int NKB>
__device__ __forceinline__ void dma_linear(const unsigned char* src, unsigned char* dst, int lane) {
#pragma unroll
  for (int i = 0; i < NKB; ++i)
    __builtin_amdgcn_global_load_lds((glb_ptr)(src + i * 1024 + lane * 16), (lds_ptr)(dst + i * 1024), 16, 0, 0);
}

}  // namespace
