// What the lane-split LayerNorm kernels share: ln_fwd_kernel / ln_bwd_kernel / pool_fwd_kernel / pool_bwd_kernel (layernorm.hip,
// the ViT widths) and ln_rows_fwd_kernel / ln_rows_bwd_kernel (swin.hip, the SwinV2 stage widths).  (ln_bwd_rows.h is the other
// layout -- rows of an LDS staging tile, 8 lanes per row -- of the fused epilogues.)
//
// Layout: LPR lanes of a wave own one row of E = NV * LPR * 4 elements, a lane holds NV vectors of 4 consecutive elements, element
// index e = (v * LPR + l) * 4 + i; a workgroup of 256 threads walks G = 256 / LPR rows per pass.  LPR = 8 / 16 / 32 keep a row
// inside one lane's registers at E <= 384; LPR = 64 puts one wave on a row (E = 512 / 768 / 1024 would not fit at 16 lanes).
// Statistics are fp32, two-pass (mean, then centred variance), held in registers.
//
// The arithmetic of one element is NOT here: each family keeps its own spelling (LnExact / LnDiv, common.h) and the forward body
// below takes it as a parameter.  The two backward kernels keep a row loop each (see ln_rows_bwd_kernel, swin.hip) and share the
// helpers only.
#pragma once
#include "common.h"

namespace ln_split {

// sum over the LPR lanes of a row, butterfly order 32, 16, 8, 4, 2, 1
template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
  static_assert(LPR == 8 || LPR == 16 || LPR == 32 || LPR == 64, "lanes per row");
  if constexpr (LPR == 8) return group8_sum(v);
  else if constexpr (LPR == 16) return group16_sum(v);
  else if constexpr (LPR == 32) return group16_sum(v + __shfl_xor(v, 16, 64));
  else return wave_sum(v);
}

template <int NV, int LPR>
struct Lanes {
  static constexpr int E = NV * LPR * 4, G = 256 / LPR;
  static __device__ __forceinline__ int lane() { return threadIdx.x & (LPR - 1); }     // position inside the row
  static __device__ __forceinline__ int group() { return threadIdx.x / LPR; }          // row group of the workgroup pass
  static __device__ __forceinline__ int col(int v, int l) { return (v * LPR + l) * 4; }

  // row: the first element of the row (or of gamma / beta)
  template <typename T>
  static __device__ __forceinline__ void load_row(const T* row, int l, f32x4 (&o)[NV]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) o[v] = load4<T>(row + col(v, l));
  }
  // Stores go out vector by vector, each right behind its arithmetic: with a whole row computed first and stored at the end the
  // compiler sank the batched loads of pool_bwd_kernel into the row turns (one exposed round trip per row again).
  template <typename T>
  static __device__ __forceinline__ void store_vec(T* row, int v, int l, f32x4 o) { store4<T>(row + col(v, l), o); }
  static __device__ __forceinline__ void zero(f32x4 (&o)[NV]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) o[v] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  // Column sums over the G row groups of the workgroup, in a fixed order (deterministic): every lane hands in its acc, store(e, sum)
  // is called once per column e by the thread that summed it.  Contains one __syncthreads; a caller that reuses red puts another
  // in front.
  template <typename StoreF>
  static __device__ __forceinline__ void col_sums(float (&red)[G][E + 4], const f32x4 (&acc)[NV], int grp, int l, StoreF&& store) {
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[grp][col(v, l) + i] = acc[v][i];
    __syncthreads();
    for (int e = threadIdx.x; e < E; e += 256) {
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < G; ++r) a += red[r][e];
      store(e, a);
    }
  }
  // the dgamma | dbeta pair of a backward: part[blk][2][E]
  static __device__ __forceinline__ void col_sums_pair(float (&red)[G][E + 4], const f32x4 (&dg)[NV], const f32x4 (&db)[NV], int grp,
                                                       int l, float* __restrict__ part, int blk) {
    for (int pass = 0; pass < 2; ++pass) {
      __syncthreads();
      f32x4 acc[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[v][i] = pass == 0 ? dg[v][i] : db[v][i];
      col_sums(red, acc, grp, l, [&](int e, float a) { part[((size_t)blk * 2 + pass) * E + e] = a; });
    }
  }
};

// ---- the forward body: y = LN(x) [* s_b] [+ res], mean / rstd saved.  A: the arithmetic of one element (common.h).
// POST: the Swin side's res-post-norm form -- res and sscale may still be null at run time (rows_per_sample rows share a scale).
template <typename A, bool POST, typename T, int NV, int LPR>
__device__ __forceinline__ void fwd_body(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                         const T* __restrict__ res, const float* __restrict__ sscale, int rows_per_sample,
                                         T* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, int M, float eps) {
  typedef Lanes<NV, LPR> L;
  constexpr int E = L::E, G = L::G;
  const int l = L::lane(), grp = L::group();
  f32x4 gm[NV], bt[NV];
  L::load_row(gamma, l, gm);
  L::load_row(beta, l, bt);
  for (int row = blockIdx.x * G + grp; row < M; row += gridDim.x * G) {
    f32x4 xv[NV], rv[NV];
    float s = 0.f, sc = 1.f;
    L::load_row(x + (size_t)row * E, l, xv);
    if constexpr (POST) {
      if (res) L::load_row(res + (size_t)row * E, l, rv);
      if (sscale) sc = sscale[row / rows_per_sample];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) s += xv[v][0] + xv[v][1] + xv[v][2] + xv[v][3];
    const float mu = A::template mean<E>(row_sum<LPR>(s));
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i) A::sq(xv[v][i], mu, q);
    const float rs = A::template rstd<E>(row_sum<LPR>(q), eps);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i] = A::norm(xv[v][i], mu, rs, gm[v][i], bt[v][i]);
        if constexpr (POST) o[i] *= sc;
      }
      if constexpr (POST) {
        if (res) {
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] += rv[v][i];
        }
      }
      L::store_vec(y + (size_t)row * E, v, l, o);
    }
    if (l == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
  }
}

// ---- host side: (dtype, E) -> (T, NV, LPR).  f is a generic lambda taking two tags, f(Type<T>{}, Shape<NV, LPR>{}) -> int; an
// unknown dtype or a width the table does not hold returns RGBNM_EINVAL without calling it.
template <typename T> struct Type { typedef T type; };
template <int NV_, int LPR_> struct Shape { static constexpr int NV = NV_, LPR = LPR_; };
enum Table {
  VIT,       // 192 / 384 at 16 lanes per row, 512 / 768 / 1024 at 64: the ViT forward and both head-pool kernels
  VIT_BWD,   // the same with 384 at 32 lanes: at 16 its six vectors per operand cost 162 VGPRs (3 waves per SIMD)
  SWIN       // 96 / 192 / 384 / 768: three vectors per lane at every width
};

template <typename F>
int for_dtype(int dtype, F&& f) {
  if (dtype == DT_BF16) return f(Type<bf16>{});
  if (dtype == DT_F32) return f(Type<float>{});
  if (dtype == DT_F16) return f(Type<f16>{});
  return RGBNM_EINVAL;
}
template <Table TABLE, typename F>
int for_width(int E, F&& f) {
  if constexpr (TABLE == SWIN) {
    if (E == 96) return f(Shape<3, 8>{});
    if (E == 192) return f(Shape<3, 16>{});
    if (E == 384) return f(Shape<3, 32>{});
    if (E == 768) return f(Shape<3, 64>{});
  } else {
    if (E == 192) return f(Shape<3, 16>{});
    if (E == 384) {
      if constexpr (TABLE == VIT_BWD) return f(Shape<3, 32>{});
      else return f(Shape<6, 16>{});
    }
    if (E == 512) return f(Shape<2, 64>{});
    if (E == 768) return f(Shape<3, 64>{});
    if (E == 1024) return f(Shape<4, 64>{});
  }
  return RGBNM_EINVAL;
}
template <Table TABLE, typename F>
int dispatch(int dtype, int E, F&& f) {
  return for_dtype(dtype, [&](auto t) { return for_width<TABLE>(E, [&](auto s) { return f(t, s); }); });
}

}  // namespace ln_split
