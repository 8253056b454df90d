// y = keep . scale . x with the dropout mask of rgbnm.h (philox.h): the encoder block backward's masked copies of its output
// gradient (site 2) and of d(x_mid) (site 0), rgbnm_vit_block_bwd_drop.  HBM-bound: one thread takes 8 consecutive columns of a
// row (two Philox counters), 16-byte loads and stores where rows allow it.
#include "common.h"
#include "../../include/rgbnm.h"
#include "philox.h"

namespace {

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dropout_apply_kernel(const T* x, int ldx, T* y, int ldy, int M,
                                                            int N, DropArgs d) {
  const unsigned long long sd = *d.seed;
  const uint32_t k0 = (uint32_t)sd, k1 = (uint32_t)(sd >> 32);
  const unsigned G = (unsigned)(N + 7) >> 3;                   // 8-column groups per row
  const unsigned total = (unsigned)M * G;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const int row = (int)(i / G), c0 = (int)(i % G) * 8;
    const uint4 w0 = drop_words(k0, k1, d.stream, row, c0 >> 2), w1 = drop_words(k0, k1, d.stream, row, (c0 >> 2) + 1);
    const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    const T* xr = x + (size_t)row * ldx + c0;
    T* yr = y + (size_t)row * ldy + c0;
    if constexpr (VEC && sizeof(T) == 2) {
      using V8 = typename Vec8<T>::type;
      V8 v = *reinterpret_cast<const V8*>(xr);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = from_f32<T>(drop_one(d, w[e], to_f32(v[e])));
      *reinterpret_cast<V8*>(yr) = v;
    } else if constexpr (VEC) {
      f32x4 a = *reinterpret_cast<const f32x4*>(xr), b = *reinterpret_cast<const f32x4*>(xr + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] = drop_one(d, w[e], a[e]);
        b[e] = drop_one(d, w[e + 4], b[e]);
      }
      *reinterpret_cast<f32x4*>(yr) = a;
      *reinterpret_cast<f32x4*>(yr + 4) = b;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (c0 + e < N) yr[e] = from_f32<T>(drop_one(d, w[e], to_f32(xr[e])));
    }
  }
}

template <typename T>
int launch_apply(const T* x, int ldx, T* y, int ldy, int M, int N, const DropArgs& d, hipStream_t st) {
  const long long total = (long long)M * ((N + 7) / 8);
  if (total >= (1LL << 31)) return RGBNM_EINVAL;
  const int grid = (int)(cdivl(total, 256) < 8192 ? cdivl(total, 256) : 8192);
  const bool vec = N % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && ((size_t)x % 16) == 0 && ((size_t)y % 16) == 0;
  if (vec) hipLaunchKernelGGL((dropout_apply_kernel<T, true>), dim3(grid), dim3(256), 0, st, x, ldx, y, ldy, M, N, d);
  else hipLaunchKernelGGL((dropout_apply_kernel<T, false>), dim3(grid), dim3(256), 0, st, x, ldx, y, ldy, M, N, d);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

}  // namespace

extern "C" int rgbnm_dropout_apply(int dtype, const void* seed, float p, int site, int block, const void* x, int ldx, void* y,
                                   int ldy, int M, int N, void* stream) {
  DropArgs d;
  if (!seed || !x || !y || M <= 0 || N <= 0 || ldx < N || ldy < N || site < 0 || site > 3 || block < 0 ||
      !drop_host_args(p, d.thr, d.scale))
    return RGBNM_EINVAL;
  d.seed = reinterpret_cast<const unsigned long long*>(seed);
  d.stream = (uint32_t)block * 4u + (uint32_t)site;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DT_BF16) return launch_apply<bf16>((const bf16*)x, ldx, (bf16*)y, ldy, M, N, d, st);
  if (dtype == DT_F16) return launch_apply<f16>((const f16*)x, ldx, (f16*)y, ldy, M, N, d, st);
  if (dtype == DT_F32) return launch_apply<float>((const float*)x, ldx, (float*)y, ldy, M, N, d, st);
  return RGBNM_EINVAL;
}
