// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC 2011) and the dropout mask
// contract of rgbnm.h (rgbnm_gemm_nt_drop, rgbnm_dropout_apply).  Every kernel that draws a dropout mask uses drop_words():
// one function, one stream of bits, so the forward epilogues and the backward's apply launches agree element for element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

// 10 rounds; key (k0, k1), counter c.  Known-answer vectors: tests/test_dropout_cpu.py (Random123's kat_vectors).
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// Dropout arguments of one launch.  seed: device pointer to the 64-bit seed (key = its low / high 32 bits), read by the kernel so
// that a captured graph replays with whatever seed the step drew; stream = block * 4 + site (counter word 2).
struct DropArgs {
  const unsigned long long* seed;
  uint32_t thr;       // keep <=> word >= thr;  thr = llround(p 2^32)
  float scale;        // 1 / (1 - p) in fp32
  uint32_t stream;
};

// the four mask words of columns 4 col4 .. 4 col4 + 3 of `row`: counter (col4, row, stream, 0); column col takes word col & 3
__device__ __forceinline__ uint4 drop_words(uint32_t k0, uint32_t k1, uint32_t stream, int row, int col4) {
  return philox4x32_10(make_uint4((uint32_t)col4, (uint32_t)row, stream, 0u), k0, k1);
}
__device__ __forceinline__ float drop_one(const DropArgs& d, uint32_t w, float v) { return w >= d.thr ? v * d.scale : 0.f; }

// host side: p in [0, 1) -> threshold / scale of the contract; false for p outside [0, 1)
inline bool drop_host_args(float p, uint32_t& thr, float& scale) {
  if (!(p >= 0.f && p < 1.f)) return false;
  const long long t = llround((double)p * 4294967296.0);
  thr = t > 0xFFFFFFFFLL ? 0xFFFFFFFFu : (uint32_t)t;
  scale = 1.0f / (1.0f - p);
  return true;
}
