// Body of the row-panel NT GEMM, included by gemm_nt_kpipe.hip once per geometry (KP_NS, KP_NWAVES, KP_NSTAGE, KP_BIAS_LDS).
namespace KP_NS {

#ifdef KP_PROF   // experiments only: cycle stamps of wave 0 of the one-tile kernel (tools/kpipe_prof.py): start, first k-tile landed, k-loop done, end
__device__ unsigned long long g_kp_prof[4096 * 4];
#define KPROF(i) do { if (tid == 0 && blockIdx.x < 4096) g_kp_prof[blockIdx.x * 4 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define KPROF(i) do { } while (0)
#endif

// Two geometries (this file is included twice by gemm_nt_kpipe.hip):
//   kp7: 7 waves x 32 rows = 224-row panels, 3-stage ring (156 KB): ONE workgroup per CU, one image per workgroup at B = 256;
//   kp8: 8 waves x 32 rows = 256-row panels, 2-stage ring (112 KB), plain epilogues: the SwinV2 row counts.
// (Round 6 pruned two measured-and-slower alternatives: the 4-wave / two-workgroups-per-CU geometry "kp_split" and the variant
// with an eighth wave issuing every LDS-DMA, "nt_dmawave"; DESIGN.md 7 keeps their numbers.)
constexpr int BN = 192, TKB = 128;            // k-tile: 64 bf16 = 128 bytes per row
constexpr int NWAVES = KP_NWAVES, NTHREADS = 64 * NWAVES, BM = 32 * NWAVES;
constexpr int A_STAGE = BM * TKB;             // 28 KB / 16 KB
constexpr int W_STAGE = BN * TKB;             // 24 KB
constexpr int STAGE = A_STAGE + W_STAGE;      // 52 KB / 40 KB
constexpr int NSTAGE = KP_NSTAGE;
constexpr int NSLOT = STAGE / 1024;           // 1 KB DMA instructions per k-tile: 52 / 40
constexpr int ASLOT = A_STAGE / 1024;         // of which A rows: 28 / 16
constexpr int NDMA = (NSLOT + NWAVES - 1) / NWAVES;   // per wave per k-tile: 8 (56 slots for 52: 4 repeats) / 10
constexpr int CP = BN + 4;                    // staging pitch (elements)
constexpr bool BIAS_LDS = KP_BIAS_LDS;
constexpr int BIAS_OFF = NSTAGE * STAGE;      // 192 floats behind the ring
constexpr int SMEM = NSTAGE * STAGE + (BIAS_LDS ? BN * 4 : 0);
constexpr int NVEC = (BM * (BN / 8) + NTHREADS - 1) / NTHREADS;      // 12 output vectors per thread
static_assert(BM * CP * 2 <= NSTAGE * STAGE, "staging tile lives in the ring");
static_assert(SMEM * (NWAVES <= 4 ? 2 : 1) <= 160 * 1024, "LDS");

enum { EPI_NONE = 0, EPI_RES = 1, EPI_LNBWD = 2, EPI_RES_LN = 3, EPI_GELU = 4, EPI_DGELU = 5 };
// LayerNorm epilogues: 8 lanes per row, lane l8 holds elements v * 64 + l8 * 8 + (0..7), v = 0..2 -- three 16-byte vectors,
// so rows move as 16 B per lane (half the vmem instructions of the 16-lane / 8-byte layout of layernorm.hip; in these
// epilogues every wave of the CU stores at once and a store costs ~200 cycles to issue).  Each lane plays the two
// "virtual" lanes 2 l8 and 2 l8 + 1 of the 16-lane layout and the reductions follow that butterfly (xor 8, 4, 2 across
// lanes, xor 1 inside the lane), so statistics and outputs keep the bits of ln_fwd_kernel / ln_bwd_kernel.
constexpr int LN_E = 192, LN_GROUPS = NTHREADS / 8, LN_ITERS = BM / LN_GROUPS;   // 56 row groups of 8 lanes, 4 rounds
// EPI_LNBWD uses the same 8-lane layout through ln_bwd_rows.h, the one implementation it shares with mlp_bwd_kernel (48 more
// accumulator registers for dgamma / dbeta than the 16-lane form it replaced; measured equal on the whole step, A/B on one box)
constexpr int RED_OFF = (BM * CP * 2 + 1023) / 1024 * 1024;   // column-reduction scratch behind the staging tile
template <typename E> using LnBwdT = rgbnm::LnBwdRows<NTHREADS, BM, E>;
typedef LnBwdT<bf16> LnBwd;                  // EPI_LNBWD: 8 lanes per row, shared with mlp_bwd_kernel (ln_bwd_rows.h)
constexpr bool LN_OK = BM * CP * 2 <= RED_OFF && RED_OFF + LnBwd::RED_BYTES <= NSTAGE * STAGE;   // LN scratch fits the ring (not kp8)

// (the 16-bit operand pointers are typed bf16 for their 2-byte address arithmetic; the plain epilogues read and write them as the
// kernel's element type E, bf16 or fp16, and so do the LayerNorm epilogues)
struct KpArgs {
  const bf16* A; const bf16* W; bf16* C; const float* bias; const bf16* R;
  int lda, ldw, ldc, ldr;
  int M, K, rows_per_wg, npanels;
  int ntiles;                  // N / 192 column tiles (LayerNorm epilogues: 1); block -> (panel, tile) map is XCD aware
  bf16* C2; int ldc2;          // EPI_GELU: C = gelu(u), C2 = gelu'(u);  EPI_DGELU: C = (A.W^T) * R
  // EPI_LNBWD: C = [R +] LayerNorm'(A.W^T) w.r.t. its input X (saved mean / rstd), partial dgamma/dbeta per panel
  const bf16* X; const float* gamma; const float* mean; const float* rstd; float* part;
  int ldx;
  // EPI_RES_LN: C = A.W^T + bias + R, then Y2 = LayerNorm(C) (gamma, beta) with its row statistics saved
  const float* beta; bf16* Y2; float* mean_o; float* rstd_o; float eps; int ldy2;
  // EPI_GELU: table GELU (gelu_table.h) when tab.img != nullptr -- the persistent kernel reloads the image behind every k-loop (it
  // shares LDS offset 0 with ring stage 0, the staging tile moves 14 KB up), the 8-wave kernel keeps it resident below its ring
  rgbnm::GeluTabKeys tab = {nullptr, 0, 0, 0, 0, 0};
};
constexpr int TAB_RESERVE = rgbnm::GELU_TAB_RESERVE;
// persistent kernel with the table: the GELU image (TAB_RESERVE bytes at LDS offset 0) + the staging tile above it must end below
// the LAST ring stage, which receives the next unit's first k-tile while the epilogue runs -- hence NSTAGE >= 3 and this bound
constexpr bool TAB_PERSIST_OK = NSTAGE >= 3 && BM * CP * 2 + TAB_RESERVE <= (NSTAGE - 1) * STAGE;
constexpr bool TAB_RESIDENT_OK = (SMEM + TAB_RESERVE) * (NWAVES <= 4 ? 2 : 1) <= 160 * 1024;   // image below the whole ring (kp8)


// The 24 MFMAs of one 64-wide k-tile with their fragment reads and this wave's DMA requests in a PINNED order
// (sched_barrier after every step): all fragments of the first 16 k, then one MFMA at a time, behind it one fragment of the next
// 16 k (into the registers an earlier MFMA has read) and, ND times per k-tile, one DMA request.  Left alone the compiler emits
// read - wait - MFMA 24 times over with two fragment registers (it minimises registers: the epilogues set the allocation), i.e.
// one exposed LDS latency per MFMA (tools/isa_scan.py) -- and
// every wave of the CU pushes its DMA requests into the texture addresser in one burst behind the barrier.  Same MFMA order per
// accumulator (k ascending): same bits.  In the step (rocprofv3, JPEG-S): fc2 / proj + residual 63.6 -> 57.1 us, fc1 + GELU 139 -> 135,
// dGELU 122 -> 116.  The 8-wave geometry (2 A + 3 W fragments per 6 MFMAs, 150 registers: the compiler already keeps a chunk of
// fragments ahead there) measured 6 % SLOWER pinned the same way and keeps the plain loop.
template <typename E, bool W2D, int ND, class DmaFn>
__device__ __forceinline__ void ktile_mma(const unsigned char* sA, const unsigned char* sW, const int (&foff)[4], int wn,
                                          f32x16 (&acc)[6], bool do_dma, DmaFn dma) {
#define KP_LD(ptr) (*reinterpret_cast<const typename Vec8<E>::type*>(ptr))
#define KP_SB __builtin_amdgcn_sched_barrier(0)
  if constexpr (!W2D) {
    KP_SB;
    Frag<E> fa[4], fb[4][6];
    fa[0].v = KP_LD(sA + foff[0]);
#pragma unroll
    for (int b = 0; b < 6; ++b) fb[0][b].v = KP_LD(sW + 32 * b * TKB + foff[0]);
    KP_SB;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const int m = c * 6 + b;
        mma(acc[b], fb[c][b], fa[c]);     // swapped: D rows <-> features, D cols <-> tokens
        KP_SB;
        if (c < 3) {
          if (b == 0) fa[c + 1].v = KP_LD(sA + foff[c + 1]);
          fb[c + 1][b].v = KP_LD(sW + 32 * b * TKB + foff[c + 1]);
        }
        if ((m * ND) / 24 != ((m + 1) * ND) / 24) {
          if (do_dma) dma((m * ND) / 24);
        }
        KP_SB;
      }
  } else {
    if (do_dma) {
#pragma unroll
      for (int j = 0; j < ND; ++j) dma(j);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      Frag<E> fa[2], fb[3];
      fa[0].v = KP_LD(sA + foff[c]);
      fa[1].v = KP_LD(sA + 32 * TKB + foff[c]);
#pragma unroll
      for (int j = 0; j < 3; ++j) fb[j].v = KP_LD(sW + (96 * wn + 32 * j) * TKB + foff[c]);
#pragma unroll
      for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int j = 0; j < 3; ++j) mma(acc[3 * rg + j], fb[j], fa[rg]);
    }
  }
#undef KP_LD
#undef KP_SB
}

template <typename E, int EPI>
__global__ __launch_bounds__(NTHREADS) void gemm_nt_kpipe_kernel(KpArgs p) {
  constexpr bool IS_BF16 = std::is_same<E, bf16>::value;      // the GELU table is a bf16 image: other types take the arithmetic GELU
  using V8 = typename Vec8<E>::type;
  using V4 = typename Vec4<E>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem0[];
  // EPI_GELU with the table (8-wave geometry: 14 KB to spare): the image stays at LDS offset 0 for the workgroup's life, ring,
  // staging tile and bias live TAB_RESERVE higher
  const bool tabr = IS_BF16 && EPI == EPI_GELU && TAB_RESIDENT_OK && p.tab.img != nullptr;
  unsigned char* const smem = smem0 + (tabr ? TAB_RESERVE : 0);
  float* Bs = reinterpret_cast<float*>(smem + BIAS_OFF);
  // blocks that share an A row panel (its column tiles) are neighbours on one XCD (block b runs on XCD b % 8): the
  // panel's k-tiles come from HBM once and from that XCD's L2 for the other tiles
  const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;
  const int panel = (jj / p.ntiles) * 8 + xcd;
  if (panel >= p.npanels) return;
  const int n0 = (jj % p.ntiles) * BN;
  const int m0 = panel * p.rows_per_wg;
  const int rows = min(p.rows_per_wg, p.M - m0);          // valid rows of this panel (<= 224)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, g = lane >> 5;
  KPROF(0);
  if (tabr) rgbnm::gelu_table_dma(p.tab.img, smem0, w, NWAVES, lane);       // (oldest in every wave's vmcnt queue: landed with k-tile 0)
  unsigned k4v = 0x00040004u;
  asm volatile("" : "+v"(k4v));


  // ---- residual rows of this panel, straight into registers (oldest loads: they never delay a k-tile wait)
  V8 rv[NVEC];
  if (EPI == EPI_RES || EPI == EPI_DGELU) {
#pragma unroll
    for (int i = 0; i < NVEC; ++i) {
      const int idx = tid + NTHREADS * i, row = idx / (BN / 8), vec = idx % (BN / 8);
      const int rr = row < rows ? row : rows - 1;
      rv[i] = *reinterpret_cast<const V8*>(p.R + (size_t)(m0 + rr) * p.ldr + n0 + vec * 8);
    }
  }
  // EPI_RES_LN: residual rows in the 8-lanes-per-row layout of its LayerNorm pass (gamma / beta: after the loop)
  const int l8 = tid & 7, grp = tid >> 3;
  V8 lr[LN_ITERS][3];
  if (EPI == EPI_RES_LN) {
#pragma unroll
    for (int it = 0; it < LN_ITERS; ++it) {
      const int row = it * LN_GROUPS + grp, rr = m0 + (row < rows ? row : rows - 1);
#pragma unroll
      for (int v = 0; v < 3; ++v)
        lr[it][v] = *reinterpret_cast<const V8*>(p.R + (size_t)rr * p.ldr + v * 64 + l8 * 8);
    }
  }
  // EPI_LNBWD: the LayerNorm input rows and their statistics, also ahead of the loop
  LnBwdT<E> lnb;
  if (EPI == EPI_LNBWD) lnb.request_x(reinterpret_cast<const E*>(p.X), p.ldx, p.mean, p.rstd, m0, rows, tid);
  if (BIAS_LDS && w < BN / 64) {
    if (p.bias) __builtin_amdgcn_global_load_lds((glb_ptr)(p.bias + n0 + 64 * w + lane), (lds_ptr)(Bs + 64 * w), 4, 0, 0);
    else Bs[64 * w + lane] = 0.f;
  }

  // ---- DMA slots: instruction i (mod NSLOT) covers 8 rows x 128 B; i < ASLOT: A rows, else W rows
  const bf16* src[NDMA];
  int dst[NDMA];
#pragma unroll
  for (int j = 0; j < NDMA; ++j) {
    int i = w + NWAVES * j;
    i = i < NSLOT ? i : i - NSLOT;
    const int r8 = (i < ASLOT ? i : i - ASLOT) * 8 + (lane >> 3), pc = lane & 7;
    const int lc = pc ^ fswz(r8);
    if (i < ASLOT) {
      const int rr = r8 < rows ? r8 : rows - 1;
      src[j] = p.A + (size_t)(m0 + rr) * p.lda + lc * 8;
      dst[j] = i * 1024;
    } else {
      src[j] = p.W + (size_t)(n0 + r8) * p.ldw + lc * 8;
      dst[j] = A_STAGE + (i - ASLOT) * 1024;
    }
  }
  int k0 = 0;
  auto issue = [&](int stage) {
    unsigned char* st = smem + stage * STAGE;
#pragma unroll
    for (int j = 0; j < NDMA; ++j) {
      __builtin_amdgcn_global_load_lds((glb_ptr)(src[j] + k0), (lds_ptr)(st + dst[j]), 16, 0, 0);
    }
    k0 += 64;
  };
  auto issue1 = [&](unsigned char* st, int j) {      // one DMA instruction of the k-tile at k0 (ktile_mma spreads them over the MFMAs)
    __builtin_amdgcn_global_load_lds((glb_ptr)(src[j] + k0), (lds_ptr)(st + dst[j]), 16, 0, 0);
  };

  // ---- fragment addresses inside a stage
  const int fl = fswz(l31);
  int foff[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) foff[c] = l31 * TKB + (((2 * c + g) ^ fl) << 4);
  // Wave tiles.  7 / 4 waves: one wave = 32 rows x all 192 columns (1 A + 6 W fragments per 6 MFMAs).  8 waves (kp8): a 4 x 2
  // grid of 64-row x 96-column wave tiles (2 A + 3 W fragments per 6 MFMAs: 29 % fewer LDS fragment reads per MFMA)
  constexpr bool W2D = NWAVES == 8;
  const int wm = W2D ? (w >> 1) : w, wn = W2D ? (w & 1) : 0;
  const int a_row = (W2D ? 64 : 32) * wm * TKB;

  f32x16 acc[6];
#pragma unroll
  for (int b = 0; b < 6; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

  const int T = p.K / 64;
  int st_issue = 0, st_comp = 0;
  // NSTAGE 3: two k-tiles ahead.  NSTAGE 2 (two workgroups per CU): one k-tile ahead -- the other workgroup of the CU
  // computes while this one waits for its tile
  constexpr int AHEAD = NSTAGE - 1;
  issue(0);
  st_issue = 1;
  if (AHEAD > 1 && T > 1) {
    issue(1);
    st_issue = 2;
  }
  for (int t = 0; t < T; ++t) {
    if (AHEAD > 1 && t + 1 < T) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();        // k-tile t landed for every wave; every wave is done with k-tile t-1
    if (t == 0) KPROF(1);
    const bool do_dma = t + AHEAD < T;
    unsigned char* stD = smem + st_issue * STAGE;
    const unsigned char* sA = smem + st_comp * STAGE + a_row;
    const unsigned char* sW = smem + st_comp * STAGE + A_STAGE;
    st_comp = st_comp == NSTAGE - 1 ? 0 : st_comp + 1;
    ktile_mma<E, W2D, NDMA>(sA, sW, foff, wn, acc, do_dma, [&](int j) { issue1(stD, j); });
    if (do_dma) {
      k0 += 64;
      st_issue = st_issue == NSTAGE - 1 ? 0 : st_issue + 1;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();          // every wave is done reading the ring: it becomes the staging tile
  KPROF(2);

  // ---- pass 1: lane = token (32 w + l31), register quad = 4 consecutive features (+ bias) -> bf16 staging tile
  E* Cs = reinterpret_cast<E*>(smem);
#pragma unroll
  for (int b = 0; b < 6; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ml = W2D ? 64 * wm + 32 * (b / 3) + l31 : 32 * w + l31;
      const int nl = (W2D ? 96 * wn + 32 * (b % 3) : 32 * b) + 8 * q + 4 * g;
      f32x4 v = {acc[b][4 * q + 0], acc[b][4 * q + 1], acc[b][4 * q + 2], acc[b][4 * q + 3]};
      if (BIAS_LDS) v += *reinterpret_cast<const f32x4*>(Bs + nl);
      else if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + n0 + nl);
      store4<E>(Cs + ml * CP + nl, v);
    }
  f32x4 gm[3][2], bt[3][2];        // EPI_RES_LN: gamma / beta of this lane's 24 elements, requested now (accumulators dead)
  if (EPI == EPI_RES_LN) {
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        gm[v][hf] = *reinterpret_cast<const f32x4*>(p.gamma + v * 64 + l8 * 8 + hf * 4);
        bt[v][hf] = *reinterpret_cast<const f32x4*>(p.beta + v * 64 + l8 * 8 + hf * 4);
      }
  }
  if (EPI == EPI_LNBWD) lnb.request_res(reinterpret_cast<const E*>(p.R), p.ldr, m0, rows, tid);   // residual gradient rows: requested now (the accumulators are dead)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (EPI == EPI_RES_LN) {
    // ---- residual add, then LayerNorm forward of the finished rows: the arithmetic of ln_fwd_kernel (layernorm.hip) --
    // same operations, same summation order, contraction off and every FMA explicit -- so both produce the same bits
#pragma clang fp contract(off)
#pragma unroll
    for (int it = 0; it < LN_ITERS; ++it) {
      const int row = it * LN_GROUPS + grp;
      if (row < rows) {
        float xv[3][8];
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const E* cp = Cs + row * CP + v * 64 + l8 * 8;           // 8-byte aligned (CP * 2 = 392)
          const V4 c0 = *reinterpret_cast<const V4*>(cp), c1 = *reinterpret_cast<const V4*>(cp + 4);
          V8 xb;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            xb[i] = from_f32<E>((float)(i < 4 ? c0[i & 3] : c1[i & 3]) + (float)lr[it][v][i]);   // the residual stream is 16-bit ...
            xv[v][i] = (float)xb[i];                                                       // ... and LayerNorm sees those values
          }
          *reinterpret_cast<V8*>(p.C + (size_t)(m0 + row) * p.ldc + v * 64 + l8 * 8) = xb;
          s0 += xv[v][0] + xv[v][1] + xv[v][2] + xv[v][3];
          s1 += xv[v][4] + xv[v][5] + xv[v][6] + xv[v][7];
        }
        const float mu = group8_pair_sum(s0, s1) * (1.f / LN_E);
        float q0 = 0.f, q1 = 0.f;
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float d0 = xv[v][i] - mu, d1 = xv[v][4 + i] - mu;
            q0 = __builtin_fmaf(d0, d0, q0);
            q1 = __builtin_fmaf(d1, d1, q1);
          }
        const float rs = rsqrtf(__builtin_fmaf(group8_pair_sum(q0, q1), 1.f / LN_E, p.eps));
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          V8 ob;
#pragma unroll
          for (int i = 0; i < 8; ++i)
            ob[i] = from_f32<E>(__builtin_fmaf((xv[v][i] - mu) * rs, gm[v][i >> 2][i & 3], bt[v][i >> 2][i & 3]));
          *reinterpret_cast<V8*>(p.Y2 + (size_t)(m0 + row) * p.ldy2 + v * 64 + l8 * 8) = ob;
        }
        if (l8 == 0) {
          p.mean_o[m0 + row] = mu;
          p.rstd_o[m0 + row] = rs;
        }
      }
    }
    return;
  }
  if (EPI == EPI_LNBWD) {
    // ---- LayerNorm backward on the staged rows + panel sums of dgamma / dbeta (ln_bwd_rows.h)
    lnb.run(Cs, CP, reinterpret_cast<E*>(p.C), p.ldc, p.gamma, p.R != nullptr, p.part, panel, reinterpret_cast<float*>(smem + RED_OFF), m0, rows, tid);
    return;
  }
  // ---- pass 2: valid rows x 24 vectors of 8 features, coalesced 384-byte rows
  E* C2 = reinterpret_cast<E*>(p.C2);
#pragma unroll
  for (int i = 0; i < NVEC; ++i) {
    const int idx = tid + NTHREADS * i, row = idx / (BN / 8), vec = idx % (BN / 8);
    if (row >= rows) continue;
    const V4 c0 = *reinterpret_cast<const V4*>(Cs + row * CP + vec * 8);
    const V4 c1 = *reinterpret_cast<const V4*>(Cs + row * CP + vec * 8 + 4);
    V8 cv = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
    if (EPI == EPI_RES) {
#pragma unroll
      for (int e = 0; e < 8; ++e) cv[e] = from_f32<E>((float)cv[e] + (float)rv[i][e]);
    }
    if (EPI == EPI_DGELU) {
#pragma unroll
      for (int e = 0; e < 8; ++e) cv[e] = from_f32<E>((float)cv[e] * (float)rv[i][e]);
    }
    if (EPI == EPI_GELU && tabr) {
      unsigned pb[4], gq[4], dq[4];
      const rgbnm::tab_u32x4 raw = __builtin_bit_cast(rgbnm::tab_u32x4, cv);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) pb[jj] = raw[jj];
      rgbnm::gelu_table_pairs4(pb, gq, dq, p.tab, k4v);
      const rgbnm::tab_u32x4 gr = {gq[0], gq[1], gq[2], gq[3]}, dr = {dq[0], dq[1], dq[2], dq[3]};
      cv = __builtin_bit_cast(V8, gr);
      store_c2(C2 + (size_t)(m0 + row) * p.ldc2 + n0 + vec * 8, __builtin_bit_cast(V8, dr));
    } else if (EPI == EPI_GELU) {     // one erfc / exp2 evaluation yields gelu(u) (-> C) and gelu'(u) (-> C2), as in gemm.hip
      V8 dv;
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        const f32x2 u = {(float)cv[e], (float)cv[e + 1]};
        f32x2 gv, dgv;
        gelu_pair_fast(u, gv, dgv);
        dv[e] = from_f32<E>(dgv[0]);
        dv[e + 1] = from_f32<E>(dgv[1]);
        cv[e] = from_f32<E>(gv[0]);
        cv[e + 1] = from_f32<E>(gv[1]);
      }
      store_c2(C2 + (size_t)(m0 + row) * p.ldc2 + n0 + vec * 8, dv);
    }
    *reinterpret_cast<V8*>(p.C + (size_t)(m0 + row) * p.ldc + n0 + vec * 8) = cv;
  }
  KPROF(3);
}

// ---- persistent form of the plain epilogues (kp7 only).  Measured on the one-tile-per-workgroup kernel at E = 384 (tools/kpipe_prof.py):
// of a workgroup's life 18 - 20 % passes between its launch and the first k-tile landing, 21 - 34 % in the epilogue, and at one
// workgroup per CU nothing overlaps either.  Here a workgroup walks a contiguous range of (row panel, column tile) units and requests
// the NEXT unit's first k-tile -- into the LAST ring stage (NSTAGE - 1), which neither the 88 KB staging tile nor the GELU table image
// below it (TAB_PERSIST_OK) ever touches -- before it starts the epilogue of
// the current one: from the second unit on the prologue is gone.  Same MFMA order per output as the kernel above (same bits).
template <typename E, int EPI>
__global__ __launch_bounds__(NTHREADS) void gemm_nt_kpipe_persist_kernel(KpArgs p) {
  static_assert(EPI == EPI_NONE || EPI == EPI_RES || EPI == EPI_GELU || EPI == EPI_DGELU, "plain epilogues");
  constexpr bool IS_BF16 = std::is_same<E, bf16>::value;      // the GELU table is a bf16 image
  using V8 = typename Vec8<E>::type;
  using V4 = typename Vec4<E>::type;
  E* C2 = reinterpret_cast<E*>(p.C2);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Bs = reinterpret_cast<float*>(smem + BIAS_OFF);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, g = lane >> 5;
  const bool tab = IS_BF16 && EPI == EPI_GELU && TAB_PERSIST_OK && p.tab.img != nullptr;
  unsigned k4v = 0x00040004u;                 // (table GELU: a VGPR operand of the packed key arithmetic)
  asm volatile("" : "+v"(k4v));
  // Unit order.  Workgroup b runs on XCD b % 8 and is slot b / 8 of it; the XCD's units are numbered jj = (its panel index) *
  // ntiles + tile, and slot s takes jj = s, s + slots, ...: at any time the slots of an XCD work on CONSECUTIVE jj -- the column
  // tiles of the same few row panels -- so a panel's k-tiles come from HBM once and from that XCD's L2 for its other tiles (a
  // workgroup walking all tiles of its own panel re-read 172 - 688 KB per tile after 32 such panels had passed through a 4 MB L2).
  const int xcd = blockIdx.x & 7, slots = gridDim.x >> 3;
  const int J = ((p.npanels + 7) >> 3) * p.ntiles;            // units of an XCD (some past the last panel for xcd > npanels % 8)
  auto unit_ok = [&](int jj) { return jj < J && (jj / p.ntiles) * 8 + xcd < p.npanels; };
  int u0 = (int)(blockIdx.x >> 3);
  while (u0 < J && !unit_ok(u0)) u0 += slots;
  if (u0 >= J) return;

  // DMA slots of this wave: instruction i covers 8 rows x 128 B; i < ASLOT: A rows, else W rows (i is wave-uniform: scalar).
  // Per unit only an element offset per slot is kept (the pointer pairs and the slot geometry of the kernel above cost the
  // residual epilogues 40 bytes of scratch here, where the next unit's offsets are live through the epilogue)
  unsigned off[NDMA];
  auto set_unit = [&](int u, int& m0, int& n0, int& rows) {
    const int panel = (u / p.ntiles) * 8 + xcd;
    n0 = (u % p.ntiles) * BN;
    m0 = panel * p.rows_per_wg;
    rows = min(p.rows_per_wg, p.M - m0);
    const int ln = lane_id_here();      // opaque: the slot geometry is re-derived here, not hoisted out of the unit loop and spilled
#pragma unroll
    for (int j = 0; j < NDMA; ++j) {
      int i = w + NWAVES * j;
      i = i < NSLOT ? i : i - NSLOT;
      const int r8 = (i < ASLOT ? i : i - ASLOT) * 8 + (ln >> 3);
      const int lc = ((ln & 7) ^ fswz(r8)) * 8;
      if (i < ASLOT) off[j] = (unsigned)(m0 + (r8 < rows ? r8 : rows - 1)) * (unsigned)p.lda + lc;
      else off[j] = (unsigned)(n0 + r8) * (unsigned)p.ldw + lc;
    }
  };
  auto issue = [&](int stage, int k0) {
    unsigned char* st = smem + stage * STAGE;
#pragma unroll
    for (int j = 0; j < NDMA; ++j) {
      int i = w + NWAVES * j;
      i = i < NSLOT ? i : i - NSLOT;
      const bf16* base = i < ASLOT ? p.A : p.W;
      const int dst = i < ASLOT ? i * 1024 : A_STAGE + (i - ASLOT) * 1024;
      __builtin_amdgcn_global_load_lds((glb_ptr)(base + (size_t)off[j] + k0), (lds_ptr)(st + dst), 16, 0, 0);
    }
  };
  const int fl = fswz(l31);
  int foff[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) foff[c] = l31 * TKB + (((2 * c + g) ^ fl) << 4);
  const int a_row = 32 * w * TKB;
  const int T = p.K / 64;

  int m0, n0, rows;
  set_unit(u0, m0, n0, rows);
  int first = 0;                    // ring stage of this unit's k-tile 0
#ifdef KP_PROF
  int ui = 0;
#define KPROFU(i) do { if (tid == 0 && blockIdx.x < 256 && ui < 8) g_kp_prof[(blockIdx.x * 8 + ui) * 4 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define KPROFU(i) do { } while (0)
#endif
  bool landed0 = false;             // k-tile 0 already requested (by the previous unit's epilogue)
#pragma unroll 1
  for (int u = u0; u < J;) {
    int un = u + slots;                      // this workgroup's next unit (past J: none)
    KPROFU(0);
    while (un < J && !unit_ok(un)) un += slots;
    if (w < BN / 64) {
      if (p.bias) __builtin_amdgcn_global_load_lds((glb_ptr)(p.bias + n0 + 64 * w + lane), (lds_ptr)(Bs + 64 * w), 4, 0, 0);
      else Bs[64 * w + lane] = 0.f;
    }
    if (!landed0) issue(first, 0);
    int st_issue = first == NSTAGE - 1 ? 0 : first + 1, st_comp = first;
    if (T > 1) {
      issue(st_issue, 64);
      st_issue = st_issue == NSTAGE - 1 ? 0 : st_issue + 1;
    }
    f32x16 acc[6];
#pragma unroll
    for (int b = 0; b < 6; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    // residual rows of this unit: requested behind the barrier of the LAST k-tile (they fly under its 24 MFMAs, the end-of-loop
    // barrier and pass 1; in front of the whole k-loop, as in the kernel above, their 48 registers do not fit this kernel's loop;
    // behind the k-loop they were slower): dGELU 117.7 -> 115.2 us, fc2 / proj + residual 56.6 -> 56.2 in the JPEG-S step.
    V8 rv[NVEC];
    const int tl = 64 * w + lane_id_here();        // (opaque thread id: see set_unit)
    auto request_rows = [&]() {
      if (EPI == EPI_RES || EPI == EPI_DGELU) {
#pragma unroll
        for (int i = 0; i < NVEC; ++i) {
          const int idx = tl + NTHREADS * i, row = idx / (BN / 8), vec = idx % (BN / 8);
          const int rr = row < rows ? row : rows - 1;
          rv[i] = *reinterpret_cast<const V8*>(p.R + (size_t)(m0 + rr) * p.ldr + n0 + vec * 8);
        }
      }
    };
    auto ktile = [&](int t, bool last) {
      if (!last) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");    // everything but the youngest k-tile's DMAs
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (last) request_rows();
      const bool do_dma = t + 2 < T;
      unsigned char* stD = smem + st_issue * STAGE;
      const int kD = (t + 2) * 64;
      const unsigned char* sA = smem + st_comp * STAGE + a_row;
      const unsigned char* sW = smem + st_comp * STAGE + A_STAGE;
      st_comp = st_comp == NSTAGE - 1 ? 0 : st_comp + 1;
      ktile_mma<E, false, NDMA>(sA, sW, foff, 0, acc, do_dma, [&](int j) {
        int i = w + NWAVES * j;
        i = i < NSLOT ? i : i - NSLOT;
        const bf16* base = i < ASLOT ? p.A : p.W;
        const int dst = i < ASLOT ? i * 1024 : A_STAGE + (i - ASLOT) * 1024;
        __builtin_amdgcn_global_load_lds((glb_ptr)(base + (size_t)off[j] + kD), (lds_ptr)(stD + dst), 16, 0, 0);
      });
      if (do_dma) st_issue = st_issue == NSTAGE - 1 ? 0 : st_issue + 1;
    };
    if constexpr (EPI == EPI_RES || EPI == EPI_DGELU) {      // (the last k-tile peeled: rv is written in ONE place)
#pragma unroll 1
      for (int t = 0; t + 1 < T; ++t) ktile(t, false);
      ktile(T - 1, true);
    } else {
#pragma unroll 1
      for (int t = 0; t < T; ++t) ktile(t, t + 1 == T);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // every wave is done reading the ring: it becomes the staging tile
    KPROFU(1);
    if (tab) rgbnm::gelu_table_dma(p.tab.img, smem, w, NWAVES, lane_id_here());     // (ring stage 0 is free: the k-loop is over)
    // ---- the next unit's first k-tile, into the stage the staging tile leaves alone
    const int cm0 = m0, cn0 = n0, crows = rows;
    landed0 = false;
    if (un < J) {
      set_unit(un, m0, n0, rows);
      issue(NSTAGE - 1, 0);
      landed0 = true;
      first = NSTAGE - 1;
    }

    // ---- pass 1: lane = token, register quad = 4 consecutive features (+ bias) -> bf16 staging tile
    E* Cs = reinterpret_cast<E*>(smem + (tab ? TAB_RESERVE : 0));
    const int ml = 32 * w + l31;
#pragma unroll
    for (int b = 0; b < 6; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nl = 32 * b + 8 * q + 4 * g;
        f32x4 v = {acc[b][4 * q + 0], acc[b][4 * q + 1], acc[b][4 * q + 2], acc[b][4 * q + 3]};
        v += *reinterpret_cast<const f32x4*>(Bs + nl);
        store4<E>(Cs + ml * CP + nl, v);
      }
    if (tab) {                               // this wave's pieces of the table image (older than the prefetched k-tile) have landed
      if (landed0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    KPROFU(2);
    // ---- pass 2: valid rows x 24 vectors of 8 features, coalesced 384-byte rows
#pragma unroll
    for (int i = 0; i < NVEC; ++i) {
      const int idx = tl + NTHREADS * i, row = idx / (BN / 8), vec = idx % (BN / 8);
      if (row >= crows) continue;
      const V4 c0 = *reinterpret_cast<const V4*>(Cs + row * CP + vec * 8);
      const V4 c1 = *reinterpret_cast<const V4*>(Cs + row * CP + vec * 8 + 4);
      V8 cv = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
      if (EPI == EPI_RES) {
#pragma unroll
        for (int e = 0; e < 8; ++e) cv[e] = from_f32<E>((float)cv[e] + (float)rv[i][e]);
      }
      if (EPI == EPI_DGELU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) cv[e] = from_f32<E>((float)cv[e] * (float)rv[i][e]);
      }
      if (EPI == EPI_GELU && tab) {
        unsigned pb[4], gq[4], dq[4];
        const rgbnm::tab_u32x4 raw = __builtin_bit_cast(rgbnm::tab_u32x4, cv);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) pb[jj] = raw[jj];
        rgbnm::gelu_table_pairs4(pb, gq, dq, p.tab, k4v);
        const rgbnm::tab_u32x4 gr = {gq[0], gq[1], gq[2], gq[3]}, dr = {dq[0], dq[1], dq[2], dq[3]};
        cv = __builtin_bit_cast(V8, gr);
        store_c2(C2 + (size_t)(cm0 + row) * p.ldc2 + cn0 + vec * 8, __builtin_bit_cast(V8, dr));
      } else if (EPI == EPI_GELU) {
        V8 dv;
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const f32x2 uu = {(float)cv[e], (float)cv[e + 1]};
          f32x2 gv, dgv;
          gelu_pair_fast(uu, gv, dgv);
          dv[e] = from_f32<E>(dgv[0]);
          dv[e + 1] = from_f32<E>(dgv[1]);
          cv[e] = from_f32<E>(gv[0]);
          cv[e + 1] = from_f32<E>(gv[1]);
        }
        store_c2(C2 + (size_t)(cm0 + row) * p.ldc2 + cn0 + vec * 8, dv);
      }
      *reinterpret_cast<V8*>(p.C + (size_t)(cm0 + row) * p.ldc + cn0 + vec * 8) = cv;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // the staging tile and the bias are read: the next unit may overwrite stages 0 / 1 and Bs
    KPROFU(3);
#ifdef KP_PROF
    ++ui;
#endif
    u = un;
  }
}

template <typename E, int EPI>
int launch_persist(const KpArgs& p, hipStream_t st) {
  static DevOnce attr;
  if (attr.need()) {
    if (hipFuncSetAttribute((const void*)gemm_nt_kpipe_persist_kernel<E, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM) != hipSuccess)
      return RGBNM_ELAUNCH;
    attr.done();
  }
  const int J = ((p.npanels + 7) / 8) * p.ntiles;             // units per XCD
  const int slots = J < 32 ? J : 32;                          // 32 CUs per XCD, one workgroup each
  hipLaunchKernelGGL((gemm_nt_kpipe_persist_kernel<E, EPI>), dim3(8 * slots), dim3(NTHREADS), SMEM, st, p);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

template <typename E, int EPI>
int launch(const KpArgs& p, hipStream_t st) {
  static DevOnce attr;
  if (attr.need()) {
    if (hipFuncSetAttribute((const void*)gemm_nt_kpipe_kernel<E, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            SMEM + (TAB_RESIDENT_OK ? TAB_RESERVE : 0)) != hipSuccess)
      return RGBNM_ELAUNCH;
    attr.done();
  }
  const bool tabr = std::is_same<E, bf16>::value && EPI == EPI_GELU && TAB_RESIDENT_OK && p.tab.img != nullptr;
  hipLaunchKernelGGL((gemm_nt_kpipe_kernel<E, EPI>), dim3(cdiv(p.npanels, 8) * 8 * p.ntiles), dim3(NTHREADS),
                     SMEM + (tabr ? TAB_RESERVE : 0), st, p);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

constexpr int WG_PER_CU = NWAVES <= 4 ? 2 : 1;

// x = A . W^T + bias + R ; y = LayerNorm(x): fc2 (+ the next block's LN1) and proj (+ LN2) in one launch each.
template <typename E>
int launch_res_ln(const void* A, int lda, const void* W, int ldw, const float* bias, const void* R,
                                 int ldr, void* x, int ldc, const float* gamma, const float* beta, void* y, int ldy,
                                 float* mean, float* rstd, float eps, int M, int N, int K, hipStream_t st) {
  if constexpr (!LN_OK) return 1;
  if (N != BN || K % 64 || K < 128 || lda % 8 || ldw % 8 || ldc % 8 || ldr % 8 || ldy % 8 || M < 8192) return 1;
  KpArgs p;
  p.A = (const bf16*)A; p.W = (const bf16*)W; p.C = (bf16*)x; p.bias = bias; p.R = (const bf16*)R;
  p.lda = lda; p.ldw = ldw; p.ldc = ldc; p.ldr = ldr; p.M = M; p.K = K;
  p.X = nullptr; p.mean = p.rstd = nullptr; p.part = nullptr; p.ldx = 0;
  p.gamma = gamma; p.beta = beta; p.Y2 = (bf16*)y; p.mean_o = mean; p.rstd_o = rstd; p.eps = eps; p.ldy2 = ldy;
  p.ntiles = 1; p.C2 = nullptr; p.ldc2 = 0;
  int rows = cdiv(M, 256 * WG_PER_CU);
  if (rows > BM) rows = BM;
  p.rows_per_wg = rows;
  p.npanels = cdiv(M, rows);
  const double mn = (double)M * N;
  const int slot = rgbnm_trace_begin(TR_NT, 2.0 * mn * K, ((double)M * K + (double)N * K) * 2.0 + mn * 2.0 * 3.0, st);
  const int rc = launch<E, EPI_RES_LN>(p, st);
  rgbnm_trace_end(slot, st);
  return rc;
}

// dx = [dres +] LayerNorm'(A . W^T): the dX GEMM of fc1 / qkv with the LayerNorm backward fused into its epilogue
// (saves writing and re-reading the [M,192] gradient and one launch).  part: [npanels][2][192] partial dgamma/dbeta;
// *npanels_out tells the caller how many slices to reduce.  Returns 1 when the shape is not eligible.
template <typename E>
int launch_lnbwd(const void* A, int lda, const void* W, int ldw, const void* X, int ldx,
                                const float* gamma, const float* mean, const float* rstd, const void* dres, int ldr,
                                void* dx, int ldc, float* part, int* npanels_out, int M, int N, int K, hipStream_t st) {
  if constexpr (!LN_OK) return 1;
  if (N != BN || K % 64 || K < 256 || lda % 8 || ldw % 8 || ldc % 8 || ldx % 8 || (dres && ldr % 8) || M < 8192) return 1;
  KpArgs p;
  p.A = (const bf16*)A; p.W = (const bf16*)W; p.C = (bf16*)dx; p.bias = nullptr; p.R = (const bf16*)dres;
  p.lda = lda; p.ldw = ldw; p.ldc = ldc; p.ldr = ldr; p.M = M; p.K = K;
  p.X = (const bf16*)X; p.gamma = gamma; p.mean = mean; p.rstd = rstd; p.part = part; p.ldx = ldx;
  p.beta = nullptr; p.Y2 = nullptr; p.mean_o = p.rstd_o = nullptr; p.eps = 0.f; p.ldy2 = 0;
  p.ntiles = 1; p.C2 = nullptr; p.ldc2 = 0;
  int rows = cdiv(M, 256 * WG_PER_CU);
  if (rows > BM) rows = BM;
  p.rows_per_wg = rows;
  p.npanels = cdiv(M, rows);
  *npanels_out = p.npanels;
  const double mn = (double)M * N;
  const int slot = rgbnm_trace_begin(TR_NT, 2.0 * mn * K, ((double)M * K + (double)N * K) * 2.0 + mn * 2.0 * (dres ? 3.0 : 2.0), st);
  const int rc = launch<E, EPI_LNBWD>(p, st);
  rgbnm_trace_end(slot, st);
  return rc;
}

// returns 1 when the shape is not eligible (caller falls back to the tile-per-workgroup kernel)
template <typename E>
int launch_plain(int epi, const void* A, int lda, const void* W, int ldw, void* C, int ldc, const float* bias,
                          const void* R, int ldr, void* C2, int ldc2, int M, int N, int K, hipStream_t st) {
  // epi uses the numbering of gemm.hip: 0 none, 1 residual, 2 GELU (+ GELU' into C2), 4 dGELU product
  if (N % BN || K % 64 || K < 256 || lda % 8 || ldw % 8 || ldc % 8 || M < 8192) return 1;
  if (epi != 0 && epi != 1 && epi != 2 && epi != 4) return 1;
  if ((epi == 1 || epi == 4) && (!R || ldr % 8)) return 1;
  if (epi == 2 && (!C2 || ldc2 % 8)) return 1;
  KpArgs p;
  p.A = (const bf16*)A; p.W = (const bf16*)W; p.C = (bf16*)C; p.bias = bias; p.R = (const bf16*)R;
  p.lda = lda; p.ldw = ldw; p.ldc = ldc; p.ldr = ldr; p.M = M; p.K = K;
  p.X = nullptr; p.gamma = p.mean = p.rstd = nullptr; p.part = nullptr; p.ldx = 0;
  p.beta = nullptr; p.Y2 = nullptr; p.mean_o = p.rstd_o = nullptr; p.eps = 0.f; p.ldy2 = 0;
  p.C2 = (bf16*)C2; p.ldc2 = ldc2;
  if (epi == 2 && std::is_same<E, bf16>::value) rgbnm::gelu_table_keys(p.tab);      // fp16: tab keeps KpArgs' initialiser (img == nullptr): the arithmetic GELU runs
  p.ntiles = N / BN;
  // N = 192: one panel per CU when it fits (M / 256 rows, at most 224: one balanced round).  Several column tiles: full
  // 224-row panels (the workgroup's arithmetic intensity against the L2 -> CU fabric is what bounds these shapes)
  int rows = p.ntiles == 1 ? cdiv(M, 256 * WG_PER_CU) : BM;
  if (rows > BM) rows = BM;
  p.rows_per_wg = rows;
  p.npanels = cdiv(M, rows);
  const double mn = (double)M * N;
  const int slot = rgbnm_trace_begin(TR_NT, 2.0 * mn * K, ((double)M * K + (double)N * K) * 2.0 + mn * 2.0 +
                                                              (epi != 0 ? mn * 2.0 : 0.0), st);
  int rc;
  if (NSTAGE == 3 && BIAS_LDS && p.ntiles > 1 && rgbnm_get_option("kp_persist"))
    rc = epi == 1 ? launch_persist<E, EPI_RES>(p, st) : epi == 2 ? launch_persist<E, EPI_GELU>(p, st)
       : epi == 4 ? launch_persist<E, EPI_DGELU>(p, st) : launch_persist<E, EPI_NONE>(p, st);
  else
    rc = epi == 1 ? launch<E, EPI_RES>(p, st) : epi == 2 ? launch<E, EPI_GELU>(p, st)
       : epi == 4 ? launch<E, EPI_DGELU>(p, st) : launch<E, EPI_NONE>(p, st);
  rgbnm_trace_end(slot, st);
  return rc;
}

}  // namespace KP_NS
