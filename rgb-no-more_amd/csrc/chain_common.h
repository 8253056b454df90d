// What the two one-launch encoder kernels (vit_chain.hip, vit_chain_bwd.hip) share: a token's 192 features as MFMA operand
// fragments, and the 64 x 192 weight-chunk GEMM step over them.
#pragma once
#include "tile128.h"

namespace {

// ---- D-layout rows: 12 pieces (index c = 2 b + hs) of 8 bf16 = features 16 c + 8 g + (0..7) of the lane's token, held as PACKED
// dwords (element j of a piece = half j & 1 of dword j >> 1): as bf16 vectors built element by element the compiler kept the
// 96 values of a row set in 96 registers and spilled them
struct Rows { u32x4 v[12]; };

// Both 32-row halves (ht = 0, 1) of a 64 x 192 chunk times x as ONE stream of 24 MFMAs with the weight fragments requested
// DEPTH MFMAs ahead; chunk rows are 384 B, 16-byte chunks swizzled by pchunk (as the W1 stage of mlp_fused.hip).  Left to itself
// the scheduler (256 registers: "minimum pressure" everywhere) emits read -> wait -> MFMA with a single fragment buffer, i.e. one
// exposed LDS latency (100+ cycles under load) per 32-cycle MFMA; two waves per SIMD hide half of it at best.  The order is pinned
// with sched_group_barrier, the compiler counts the lgkmcnt values.  FENCE: close the pinned region with a sched_barrier (the backward)
template <int DEPTH, bool FENCE = false>
__device__ __forceinline__ void gemm_k192x2(f32x16& a0, f32x16& a1, const unsigned char* sW, const Rows& x, const Geo& L) {
  constexpr int WROW = 192 * 2;
  int wb0 = L.l31 * WROW + ((L.g ^ L.fl) << 4);
  asm volatile("" : "+v"(wb0));
  const int wb1 = wb0 + 32 * WROW;
  Frag<bf16> fb[24];
#pragma unroll
  for (int i = 0; i < 24; ++i) {
    const int c = i >> 1;
    fb[i].v = *reinterpret_cast<const bf16x8*>(sW + ((((i & 1) ? wb1 : wb0) ^ ((c % 4) << 5)) + 128 * (c / 4)));
  }
#pragma unroll
  for (int i = 0; i < 24; ++i) {
    Frag<bf16> fx;
    fx.v = as_bf16x8(x.v[i >> 1]);
    mma((i & 1) ? a1 : a0, fb[i], fx);
  }
  __builtin_amdgcn_sched_group_barrier(0x100, DEPTH, 0);
#pragma unroll
  for (int i = 0; i < 24 - DEPTH; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
  }
#pragma unroll
  for (int i = 0; i < DEPTH; ++i) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
  if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
}

}  // namespace
