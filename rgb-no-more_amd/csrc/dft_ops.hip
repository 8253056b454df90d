// DFT-plane Rotate / ShearX / ShearY of RandAugment_dct, batched (reference utils/dct_ops.py:367-434, 957-1013,
// utils/dct_torch_utils.py:232-321; the tensor path of this repo: dct_ops._dft_plane_op).
//
// One plane of one sample (Hb x Hb blocks of 8 x 8, zero-padded to Hp x Hp, N = 8 Hp pixels a side):
//   X = blockshift(quarter turns(pad(x)))            index and sign work, folded into stage 0's operand load
//   P = L . X                                        stage 0   (2 real N^3 products)
//   F = P . M^H                                      stage 1   (4)
//   G[p] = F[map[p]] or 0                            the composed fftshift / nearest sampling / ifftshift map, folded into stage 2's load
//   Q = L^H . G                                      stage 2   (4)
//   y = Re(Q . M)                                    stage 3   (2) -> iblockshift, crop, rint [, clamp], int16: folded into the store
// L = M = generate_conversion_matrix_dft(8, Hp).  The reference multiplies by sqrt(N) and divides by it again around each product
// pair; on square grids the factors cancel and are left out.
//
// Every stage is ONE launch over all (job, plane, 64 x 64 output tile) triples; the complex intermediates go through the
// workspace and the stages meet only at launch boundaries.  A workgroup is four waves, wave w owns rows 16 w .. 16 w + 15 of the
// tile as four 16 x 16 accumulator pairs (real, imaginary) of the exact f32-input MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf
// chain, so a tile's bits depend on its own operands only -- not on the batch, not on the run).  Operand tiles are staged through
// LDS k-major ([32][64], pitch 80 floats: the four k rows of a fragment read fall on disjoint banks) and fetched into registers one
// k tile ahead.  Every load and store is guarded against N, which need not be a multiple of anything but 8, and out-of-range
// operands are zeros (fma(0, 0, acc) = acc): the product loop itself tests no edge.
#include "common.h"
#include "internal.h"
#include "../../include/rgbnm.h"

#include <vector>

namespace dftops {

constexpr int TM = 64;        // output tile side
constexpr int KT = 32;        // reduction tile
constexpr int PITCH = 80;     // LDS row pitch in floats (80 = 16 mod 64)
constexpr int THREADS = 256;
constexpr int EL = TM * KT / THREADS;      // elements of an operand tile per thread

struct Plane {                // one (job, plane) of a launch, derived in the kernel from the job record
  int16_t* x;                 // the plane's Hb x Hb x 64 coefficients
  const float* conv;          // L, interleaved complex64 [N][N]
  const int32_t* map;         // [N * N]
  float* ws;                  // 4 N^2 floats: buffer A (re, im), buffer B (re, im)
  int Hb, Hp, N, rot, tiles;
};

struct Args {
  int16_t* Y;
  int16_t* C;
  const rgbnm_dft_job* jobs;
  const float* conv_y;
  const float* conv_c;
  const int32_t* maps_y;
  const int32_t* maps_c;
  float* ws;
  int S, Hp_y, Hp_c, ty, tc, clamp;
};

__device__ __forceinline__ void pick_plane(const Args& a, int job, int t, Plane& p, int& tile) {
  const rgbnm_dft_job jb = a.jobs[job];
  const int Ny = 8 * a.Hp_y, Nc = 8 * a.Hp_c;
  const size_t per_job = (size_t)4 * ((size_t)Ny * Ny + 2 * (size_t)Nc * Nc);
  float* ws = a.ws + (size_t)job * per_job;
  const int ntile_y = a.ty * a.ty, ntile_c = a.tc * a.tc;
  if (t < ntile_y) {
    p.x = a.Y + (size_t)jb.sample * a.S * a.S * 64;
    p.conv = a.conv_y;
    p.map = a.maps_y + (size_t)jb.map_y * Ny * Ny;
    p.ws = ws;
    p.Hb = a.S; p.Hp = a.Hp_y; p.N = Ny; p.tiles = a.ty;
    tile = t;
  } else {
    const int u = t - ntile_y;
    const int pl = u / ntile_c;             // 0: Cb, 1: Cr
    const int Sc = a.S / 2;
    p.x = a.C + ((size_t)jb.sample * 2 + pl) * Sc * Sc * 64;
    p.conv = a.conv_c;
    p.map = a.maps_c + (size_t)jb.map_c * Nc * Nc;
    p.ws = ws + (size_t)4 * Ny * Ny + (size_t)pl * 4 * Nc * Nc;
    p.Hb = Sc; p.Hp = a.Hp_c; p.N = Nc; p.tiles = a.tc;
    tile = u - pl * ntile_c;
  }
  p.rot = jb.rot90s;
}

// X[r][c] of stage 0: the padded, quarter-turned, block-shifted plane as fp32
__device__ __forceinline__ float load_x(const Plane& p, int r, int c) {
  const int Hp = p.Hp;
  int bi = (r >> 3) - (Hp >> 1), bj = (c >> 3) - (Hp >> 1);      // blockshift: roll by Hp / 2
  bi += bi < 0 ? Hp : 0;
  bj += bj < 0 ? Hp : 0;
  int u = r & 7, v = c & 7;
  int si = bi, sj = bj, su = u, sv = v;
  bool neg = false;
  // rotate_dct_90deg of the padded grid, read backwards (dct_ops.py:99-130)
  if (p.rot == 1) { si = bj; sj = Hp - 1 - bi; su = v; sv = u; neg = u & 1; }
  else if (p.rot == 2) { si = Hp - 1 - bi; sj = Hp - 1 - bj; neg = (u + v) & 1; }
  else if (p.rot == 3) { si = Hp - 1 - bj; sj = bi; su = v; sv = u; neg = v & 1; }
  const int m = (Hp - p.Hb) >> 1;
  si -= m;
  sj -= m;
  if (si < 0 || si >= p.Hb || sj < 0 || sj >= p.Hb) return 0.f;
  const float val = (float)p.x[((size_t)si * p.Hb + sj) * 64 + su * 8 + sv];
  return neg ? -val : val;
}

// y[r][c] of stage 3 -> its int16 home: iblockshift, crop, round half to even [, clamp]
__device__ __forceinline__ void store_y(const Plane& p, int r, int c, float val, int clamp) {
  const int Hp = p.Hp;
  const int t = Hp - (Hp >> 1);
  int bi = (r >> 3) + t, bj = (c >> 3) + t;
  bi -= bi >= Hp ? Hp : 0;
  bj -= bj >= Hp ? Hp : 0;
  const int m = (Hp - p.Hb) >> 1;
  bi -= m;
  bj -= m;
  if (bi < 0 || bi >= p.Hb || bj < 0 || bj >= p.Hb) return;
  float q = rintf(val);
  if (clamp) q = fminf(fmaxf(q, -1024.f), 1016.f);
  p.x[((size_t)bi * p.Hb + bj) * 64 + (r & 7) * 8 + (c & 7)] = (int16_t)(int)q;
}

// STAGE 0: A = L,      B = X (real)          -> buffer A        STAGE 1: A = buffer A, B = conj(M)^T -> buffer B
// STAGE 2: A = conj(L)^T, B = gather(buffer B) -> buffer A      STAGE 3: A = buffer A, B = M         -> Re -> int16 plane
template <int STAGE>
__global__ __launch_bounds__(THREADS, 2) void stage_kernel(Args a) {
  __shared__ float As_r[KT][PITCH], As_i[KT][PITCH], Bs_r[KT][PITCH], Bs_i[KT][PITCH];
  Plane p;
  int tile;
  const int nt = a.ty * a.ty + (a.C ? 2 * a.tc * a.tc : 0);
  if ((int)blockIdx.x >= nt) return;
  pick_plane(a, blockIdx.y, blockIdx.x, p, tile);
  const int N = p.N;
  const int row0 = (tile / p.tiles) * TM, col0 = (tile % p.tiles) * TM;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t NN = (size_t)N * N;
  const float* Ar = p.ws;                 // buffer A
  const float* Ai = p.ws + NN;
  const float* Br = p.ws + 2 * NN;        // buffer B
  const float* Bi = p.ws + 3 * NN;

  constexpr bool B_REAL = STAGE == 0, C_REAL = STAGE == 3;
  f32x4 cr[4], ci[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cr[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    ci[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bool row_live = row0 + 16 * w < N;          // wave-uniform: a 16-row strip wholly past the edge does no products

  // ---- operand tiles: EL elements of each per thread, fetched into registers one k tile ahead of the products (the global
  // latency runs under the MFMAs of the tile before), zeros past the edges
  float fa_r[EL], fa_i[EL], fb_r[EL], fb_i[EL];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < EL; ++i) {
      // A[row][k]
      int kk, mm;
      if (STAGE == 2) { mm = tid & 63; kk = (tid >> 6) + 4 * i; }                      // memory runs along the row index
      else { kk = tid & (KT - 1); mm = tid / KT + (THREADS / KT) * i; }                // memory runs along k
      const int gr = row0 + mm, gk = k0 + kk;
      float vr = 0.f, vi = 0.f;
      if (gr < N && gk < N) {
        if (STAGE == 0) {
          const float2 z = *reinterpret_cast<const float2*>(p.conv + 2 * ((size_t)gr * N + gk));
          vr = z.x; vi = z.y;
        } else if (STAGE == 2) {
          const float2 z = *reinterpret_cast<const float2*>(p.conv + 2 * ((size_t)gk * N + gr));
          vr = z.x; vi = -z.y;
        } else {
          vr = Ar[(size_t)gr * N + gk];
          vi = Ai[(size_t)gr * N + gk];
        }
      }
      fa_r[i] = vr;
      fa_i[i] = vi;
    }
#pragma unroll
    for (int i = 0; i < EL; ++i) {
      // B[k][col]
      int kk, nn;
      if (STAGE == 1) { kk = tid & (KT - 1); nn = tid / KT + (THREADS / KT) * i; }
      else { nn = tid & 63; kk = (tid >> 6) + 4 * i; }
      const int gc = col0 + nn, gk = k0 + kk;
      float vr = 0.f, vi = 0.f;
      if (gc < N && gk < N) {
        if (STAGE == 0) {
          vr = load_x(p, gk, gc);
        } else if (STAGE == 1) {
          const float2 z = *reinterpret_cast<const float2*>(p.conv + 2 * ((size_t)gc * N + gk));
          vr = z.x; vi = -z.y;
        } else if (STAGE == 2) {
          const int src = p.map[(size_t)gk * N + gc];
          if (src >= 0 && (size_t)src < NN) { vr = Br[src]; vi = Bi[src]; }
        } else {
          const float2 z = *reinterpret_cast<const float2*>(p.conv + 2 * ((size_t)gk * N + gc));
          vr = z.x; vi = z.y;
        }
      }
      fb_r[i] = vr;
      fb_i[i] = vi;
    }
  };
  auto stage_to_lds = [&]() {
#pragma unroll
    for (int i = 0; i < EL; ++i) {
      int kk, mm;
      if (STAGE == 2) { mm = tid & 63; kk = (tid >> 6) + 4 * i; }
      else { kk = tid & (KT - 1); mm = tid / KT + (THREADS / KT) * i; }
      As_r[kk][mm] = fa_r[i];
      As_i[kk][mm] = fa_i[i];
      if (STAGE == 1) { kk = tid & (KT - 1); mm = tid / KT + (THREADS / KT) * i; }
      else { mm = tid & 63; kk = (tid >> 6) + 4 * i; }
      Bs_r[kk][mm] = fb_r[i];
      if (!B_REAL) Bs_i[kk][mm] = fb_i[i];
    }
  };

  fetch(0);
  for (int k0 = 0; k0 < N; k0 += KT) {
    stage_to_lds();
    __syncthreads();
    if (k0 + KT < N) fetch(k0 + KT);
    if (row_live) {
      // straight-line code: no test of the column or k edge in here (the operands past an edge are zeros), so that the
      // accumulators stay where they are and the LDS reads of a k step run under the products of the step before
#pragma unroll
      for (int ks = 0; ks < KT; ks += 4) {
        const int k = ks + (lane >> 4), l15 = lane & 15;
        const float ar = As_r[k][16 * w + l15], ai = As_i[k][16 * w + l15];
        const float nai = -ai;
        float br[4], bi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          br[j] = Bs_r[k][16 * j + l15];
          if (!B_REAL) bi[j] = Bs_i[k][16 * j + l15];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          cr[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, br[j], cr[j], 0, 0, 0);
          if (B_REAL) ci[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, br[j], ci[j], 0, 0, 0);
          else if (!C_REAL) ci[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, bi[j], ci[j], 0, 0, 0);
        }
        if (!B_REAL) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            cr[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(nai, bi[j], cr[j], 0, 0, 0);
            if (!C_REAL) ci[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, br[j], ci[j], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- store: accumulator register e of a 16 x 16 tile is row 4 (lane / 16) + e, column lane % 16
  float* Or = p.ws + (STAGE == 1 ? 2 * NN : 0);
  float* Oi = Or + NN;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gc = col0 + 16 * j + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int gr = row0 + 16 * w + 4 * (lane >> 4) + e;
      if (gr < N && gc < N) {
        if (STAGE == 3) {
          store_y(p, gr, gc, cr[j][e], a.clamp);
        } else {
          Or[(size_t)gr * N + gc] = cr[j][e];
          Oi[(size_t)gr * N + gc] = ci[j][e];
        }
      }
    }
  }
}

static size_t workspace_bytes(int njobs, int Hp_y, int Hp_c) {
  if (njobs <= 0 || Hp_y <= 0 || Hp_c <= 0) return 0;
  const size_t Ny = 8 * (size_t)Hp_y, Nc = 8 * (size_t)Hp_c;
  return (size_t)njobs * 4 * (Ny * Ny + 2 * Nc * Nc) * sizeof(float);
}

}  // namespace dftops

extern "C" {

size_t rgbnm_dct_dft_workspace(int njobs, int Hp_y, int Hp_c) { return dftops::workspace_bytes(njobs, Hp_y, Hp_c); }

int rgbnm_dct_dft_ops(int16_t* Y, int16_t* C, int B, int S, int Hp_y, int Hp_c, const rgbnm_dft_job* jobs_dev,
                      const rgbnm_dft_job* jobs_host, int njobs, const float* conv_y, const float* conv_c, const int32_t* maps_y,
                      const int32_t* maps_c, int nmaps, int clamp, void* ws, size_t ws_bytes, void* stream) {
  using namespace dftops;
  if (S < 2 || S > 32 || (S & 1) || B <= 0) return RGBNM_EINVAL;
  if (Hp_y < S || Hp_y > 48 || Hp_c < S / 2 || Hp_c > 48) return RGBNM_EINVAL;
  if (njobs < 0 || clamp < 0 || clamp > 1) return RGBNM_EINVAL;
  if ((jobs_dev != nullptr) != (jobs_host != nullptr)) return RGBNM_EINVAL;
  if (njobs == 0) return RGBNM_OK;
  if (!jobs_dev || !Y || !conv_y || !maps_y || nmaps <= 0 || (C && (!conv_c || !maps_c))) return RGBNM_EINVAL;
  std::vector<char> seen((size_t)B, 0);
  for (int j = 0; j < njobs; ++j) {
    const rgbnm_dft_job& jb = jobs_host[j];
    if (jb.sample < 0 || jb.sample >= B || seen[jb.sample]) return RGBNM_EINVAL;
    seen[jb.sample] = 1;
    if (jb.rot90s < 0 || jb.rot90s > 3) return RGBNM_EINVAL;
    if (jb.map_y < 0 || jb.map_y >= nmaps || jb.map_c < 0 || jb.map_c >= nmaps) return RGBNM_EINVAL;
  }
  if (!ws || ws_bytes < workspace_bytes(njobs, Hp_y, Hp_c)) return RGBNM_EINVAL;

  Args a;
  a.Y = Y; a.C = C; a.jobs = jobs_dev; a.conv_y = conv_y; a.conv_c = conv_c; a.maps_y = maps_y; a.maps_c = maps_c;
  a.ws = (float*)ws;
  a.S = S; a.Hp_y = Hp_y; a.Hp_c = Hp_c; a.clamp = clamp;
  a.ty = cdiv(8 * Hp_y, TM);
  a.tc = cdiv(8 * Hp_c, TM);
  const int nt = a.ty * a.ty + (C ? 2 * a.tc * a.tc : 0);
  hipStream_t st = (hipStream_t)stream;
  const double Ny = 8.0 * Hp_y, Nc = 8.0 * Hp_c;
  const double flops = 12.0 * 2.0 * (Ny * Ny * Ny + (C ? 2.0 * Nc * Nc * Nc : 0.0)) * njobs;
  const int slot = rgbnm_trace_begin(TR_DFT, flops, 0.0, st);
  // jobs on grid.y (<= 65535: njobs <= B, and a batch that large has no workspace)
  for (int j0 = 0; j0 < njobs; j0 += 32768) {
    const int nj = njobs - j0 < 32768 ? njobs - j0 : 32768;
    Args b = a;
    b.jobs = jobs_dev + j0;
    b.ws = a.ws + (size_t)j0 * (workspace_bytes(1, Hp_y, Hp_c) / sizeof(float));
    const dim3 grid(nt, nj);
    stage_kernel<0><<<grid, THREADS, 0, st>>>(b);
    stage_kernel<1><<<grid, THREADS, 0, st>>>(b);
    stage_kernel<2><<<grid, THREADS, 0, st>>>(b);
    stage_kernel<3><<<grid, THREADS, 0, st>>>(b);
  }
  rgbnm_trace_end(slot, st);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

}  // extern "C"
