// Included twice by augment.hip (AUG_NS / AUG_S / AUG_LDS): S = 28 block grids (ViT pipelines, image in LDS) and
// S = 32 (SwinV2 pipeline, image in L2).  Same code, so the bit-exact tests of one size vouch for the arithmetic of both.
namespace AUG_NS {

constexpr int CMIN = -1024, CMAX = 1016;
constexpr int S_Y = AUG_S, S_C = AUG_S / 2;
constexpr int NY = S_Y * S_Y * 64;           // 50176 (S = 28) / 65536 (S = 32)
constexpr int NC1 = S_C * S_C * 64;          // per chroma plane
constexpr int NIMG = NY + 2 * NC1;           // 75264 / 98304 int16
constexpr bool IMG_IN_LDS = AUG_LDS != 0;    // S = 32: 192 KB per image does not fit LDS -> the image stays in L2

// raw != 0: the coefficients were de-quantised and clamped upstream (unit tables): pass them through unclamped, as the
// reference's crop / resize / flip classes do with whatever their predecessor in the Compose chain produced
__device__ __forceinline__ short dequant(short c, short q, int raw) {
  const short w = (short)((int)c * (int)q);   // int16 multiply WITH wrap-around (datasets.py:288)
  return raw ? w : (w < CMIN ? (short)CMIN : (w > CMAX ? (short)CMAX : w));
}
__device__ __forceinline__ short clamp_s(int v) { return (short)(v < CMIN ? CMIN : (v > CMAX ? CMAX : v)); }

// ------------------------------------------------------------------------------------------------ kernel 1
// Work is handed out by COST, not by image: a /2 image costs ~18x an identity image (A.X.A^T on the VALU against a copy), and the
// sampler's mix is 61 % /2, 33 % identity, 6 % x2 -- with one image per workgroup set the kernel ran as long as its slowest
// image (89 us) while a third of the chip idled.  Every image is a list of equal items (/2: two output blocks; identity: eight
// blocks; x2: one input block), an image's cost is items x weight, and every wave of the grid takes the items whose start falls
// into its equal share of the batch's total cost (prefix sums over the batch in LDS, recomputed by every workgroup: B loads).
// cost weights per item of a /2, an identity, a x2 image (tools/aug_prof.py).  Macros, fixed: tests/augment_ref.py reads these lines
#define AUG_K_HALF 9
#define AUG_K_ID 8
#define AUG_K_DBL 12
constexpr int UNITS = S_Y * S_Y + 2 * S_C * S_C;          // output blocks per image: 1176 (S = 28) / 1536 (S = 32)
constexpr int N_HALF = UNITS / 2, N_ID = UNITS / 8, N_DBL = UNITS / 4;
static_assert(UNITS % 8 == 0 && (S_Y * S_Y) % 2 == 0 && (S_C * S_C) % 2 == 0 && S_Y % 2 == 0 && S_C % 2 == 0, "item shapes");
constexpr int RESIZE_MAXB = 512;                          // images per launch (prefix table in the kernel arguments); launch() loops beyond
constexpr int RESIZE_LDS = 1088 + 4 * 24 * 36 * 4 + 4 * 4 * 1024 + (RESIZE_MAXB + 1) * 4 + 12;    // As | Xt2 | Tt2 | Ring | Pfx

struct ResizeArgs {
  const short* Yq; const short* Cq; const short* quant; const rgbnm_aug_params* prm; const float* A16; short* img;
  const long long* yoff; const long long* coff;     // non-null: host-cropped input, image b's crop box packed at Yq + yoff[b] / Cq + coff[b]
  int B, Hy, Wy, Hc, Wc, has_chroma, raw, clamp_out;
  // exclusive prefix sums of the images' costs, made by launch() from the host copy of the parameters.  (Until round 6 every
  // workgroup summed them itself from prm[].crop_w: 1024 workgroups x 272 line requests on the same 15 KB -- a handful of L2
  // channels -- held every wave for 15 k cycles, a sixth of its life: tools/aug_prof.py.)
  int pfx[RESIZE_MAXB + 1];
};

typedef short short8v __attribute__((ext_vector_type(8)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// acc + a.lo * x  /  acc + a.hi * x, both halves of x and acc: one v_pk_fma_f32 (IEEE fma per half) with the scalar factor taken
// from one half of a register pair by operand selection
__device__ __forceinline__ f32x2v pk_fma_lo(f32x2v a, f32x2v x, f32x2v acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(a), "v"(x));
  return acc;
}
__device__ __forceinline__ f32x2v pk_fma_hi(f32x2v a, f32x2v x, f32x2v acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(a), "v"(x));
  return acc;
}

__host__ __device__ __forceinline__ int mode_of(int crop_w) { return crop_w == 2 * S_Y ? 0 : (crop_w == S_Y ? 1 : 2); }   // 0: /2  1: identity  2: x2
__host__ __device__ __forceinline__ int cost_of(int mode) {
  return mode == 0 ? N_HALF * AUG_K_HALF : (mode == 1 ? N_ID * AUG_K_ID : N_DBL * AUG_K_DBL);
}
// output block number inside an image -> plane, block row / column (constant divisors)
__device__ __forceinline__ void unit_decode(int unit, int& pl, int& oy, int& ox) {
  if (unit < S_Y * S_Y) { pl = 0; oy = unit / S_Y; ox = unit % S_Y; }
  else { const int u2 = unit - S_Y * S_Y; pl = 1 + u2 / (S_C * S_C); const int u3 = u2 % (S_C * S_C); oy = u3 / S_C; ox = u3 % S_C; }
}

#ifdef AUG_PROF   // experiments only (tools/aug_prof.py): per-wave cycle stamps and item counts of kernel 1
__device__ unsigned long long g_aug_prof[4096 * 8];
__device__ unsigned long long g_aug_prof2[4096 * 8];     // kernel 2: [image][wave]
#endif

__global__ __launch_bounds__(256, 4) void dct_resize_kernel(ResizeArgs a_in) {
#ifdef AUG_PROF
  const unsigned long long pf_t0 = __builtin_readcyclecounter();
  unsigned long long pf_c0 = 0, pf_c1 = 0, pf_c2 = 0; int pf_n0 = 0, pf_n1 = 0, pf_n2 = 0;
#endif
  // The kernel arguments as scalars pinned in SGPRs.  Written against the argument struct itself, a per-lane choice such as
  // `pl ? a.Wc : a.Wy` is merged by the optimiser into ONE load through a per-lane pointer into the kernarg segment: a global load
  // (and an s_waitcnt vmcnt(0)) in front of every dependent address -- the identity branch ran two chained HBM-latency loads per item.
  typedef const short __attribute__((address_space(1)))* gshort_p;      // global address space survives the pinning below
  typedef const short4v __attribute__((address_space(1)))* gshort4_p;
  typedef const short8v __attribute__((address_space(1)))* gshort8_p;
  struct { gshort_p Yq; gshort_p Cq; const short* quant; const rgbnm_aug_params* prm; const float* A16; short* img;
           const long long* yoff; const long long* coff; int B, Hy, Wy, Hc, Wc, has_chroma, raw, clamp_out; } a;
  {
    unsigned long long yq = (unsigned long long)a_in.Yq, cq = (unsigned long long)a_in.Cq;
    asm volatile("" : "+s"(yq), "+s"(cq));
    a.Yq = (gshort_p)yq; a.Cq = (gshort_p)cq;
  }
  a.quant = a_in.quant; a.prm = a_in.prm; a.A16 = a_in.A16; a.img = a_in.img; a.yoff = a_in.yoff; a.coff = a_in.coff;
  a.B = a_in.B; a.Hy = a_in.Hy; a.Wy = a_in.Wy; a.Hc = a_in.Hc; a.Wc = a_in.Wc; a.has_chroma = a_in.has_chroma;
  a.raw = a_in.raw; a.clamp_out = a_in.clamp_out;
  asm volatile("" : "+s"(a.Hy), "+s"(a.Wy), "+s"(a.Hc), "+s"(a.Wc), "+s"(a.has_chroma), "+s"(a.raw), "+s"(a.clamp_out));
  constexpr int XP = 36;                                 // words per row of the pair-interleaved tiles: 32 + 4 (16-byte reads of 16 rows hit 64 distinct banks)
  // Per-wave ring of RD raw items (1 KB each) filled by LDS-DMA RD - 1 items ahead: a wave walks its items one after the other,
  // only four waves share a SIMD, and an HBM round trip under load is ~2 us against ~0.4 us of work per item -- one item of
  // register prefetch hid a fifth of it.  The DMA needs no registers, so the depth is free.
  constexpr int RD = 4;
  // LDS carved from the dynamic segment (RESIZE_LDS bytes): with static __shared__ arrays the compiler puts an s_waitcnt vmcnt(0)
  // in front of every LDS read that follows an LDS-DMA of the same wave -- it cannot see the counted waits below -- and drains the ring
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
  float (*As)[17] = reinterpret_cast<float (*)[17]>(rs_smem);                                     // [16][17]
  float (*Xt2)[16 * XP] = reinterpret_cast<float (*)[16 * XP]>(rs_smem + 1088);                   // [4]: [X column j][X row i][unit]   (x2 path: Xs[8][17])
  float (*Tt2)[8 * XP] = reinterpret_cast<float (*)[8 * XP]>(rs_smem + 1088 + 4 * 16 * XP * 4);  // [4]: [T row u][column j][unit]     (x2 path: Ts[16][17])
  unsigned char (*Ring)[RD * 1024] = reinterpret_cast<unsigned char (*)[RD * 1024]>(rs_smem + 1088 + 4 * 24 * XP * 4);
  int* Pfx = reinterpret_cast<int*>(rs_smem + 1088 + 4 * 24 * XP * 4 + 4 * RD * 1024);           // [RESIZE_MAXB + 1]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);       // wave-uniform: the per-item index and address arithmetic runs on the scalar unit
  As[tid >> 4][tid & 15] = a.A16[tid];
  for (int i = tid; i <= a_in.B; i += 256) Pfx[i] = a_in.pfx[i];      // one coalesced read of the argument segment
  __syncthreads();
#ifdef AUG_PROF
  const unsigned long long pf_t1 = __builtin_readcyclecounter();
#endif
  const int nwave = gridDim.x * 4, wave = blockIdx.x * 4 + w;
  const int total = Pfx[a.B];
  const int share = total / nwave, rem = total % nwave;
  const int lo = wave * share + min(wave, rem), hi = lo + share + (wave < rem ? 1 : 0);
  if (lo >= hi) return;
  int b = 0;
  {                                                      // largest b with Pfx[b] <= lo
    int l = 0, h = a.B - 1;
    while (l < h) {
      const int mid = (l + h + 1) >> 1;
      if (Pfx[mid] <= lo) l = mid;
      else h = mid - 1;
    }
    b = l;
  }
  float* xt = Xt2[w];
  float* tt = Tt2[w];
  unsigned char* ring = Ring[w];
  const unsigned ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)ring;     // its LDS byte address
  for (; b < a.B && Pfx[b] < hi; ++b) {
    const rgbnm_aug_params p = a.prm[b];
    const int mode = mode_of(p.crop_w);
    const int k = mode == 0 ? AUG_K_HALF : (mode == 1 ? AUG_K_ID : AUG_K_DBL);
    const int base_c = Pfx[b], end_c = min(hi, Pfx[b + 1]);
    const int j0 = (max(lo - base_c, 0) + k - 1) / k, j1 = (end_c - base_c + k - 1) / k;     // items whose start lies in [lo, hi)
    const short* q = a.quant + (size_t)b * 192;
    short* img = a.img + (size_t)b * NIMG;
    const int flip = p.flip;
#ifdef AUG_PROF
    const unsigned long long pf_m0 = __builtin_readcyclecounter();
    if (mode == 0) pf_n0 += j1 - j0; else if (mode == 1) pf_n1 += j1 - j0; else pf_n2 += j1 - j0;
#endif
    // source geometry: whole coefficient grids (origin = the crop box's corner) or, with yoff / coff, the crop box alone as the
    // host packed it (loader.DCTBatchLoader(crop_on_host=True): origin 0, row pitch = the box, only the box crossed PCIe)
    const bool packed = a.yoff != nullptr;
    const int topY = packed ? 0 : p.crop_i, leftY = packed ? 0 : p.crop_j, topC = packed ? 0 : p.crop_i / 2, leftC = packed ? 0 : p.crop_j / 2;
    const int WY = packed ? p.crop_w : a.Wy, WC = packed ? p.crop_w / 2 : a.Wc;
    const size_t planeC = packed ? (size_t)(p.crop_h / 2) * (p.crop_w / 2) * 64 : (size_t)a.Hc * a.Wc * 64;
    gshort_p baseY = packed ? a.Yq + a.yoff[b] : a.Yq + (size_t)b * a.Hy * a.Wy * 64;
    gshort_p baseC = packed ? a.Cq + (a.has_chroma ? a.coff[b] : 0) : a.Cq + (size_t)b * 2 * planeC;
    if (mode == 0) {
      // ---- /2: item = output blocks 2 j, 2 j + 1 (same plane, same block row).  X = 2x2 input blocks gathered block-major
      // (dct_ops.py:519), T = A[0:8,:] . X, Z = T . A[0:8,:]^T / 2 -- the two units of an item ride in the two halves of packed
      // fp32 FMAs (v_pk_fma_f32: same IEEE fma per half, same summation order as one unit at a time).
      // /2: rows 2 ug, 2 ug + 1 (T phase) and row v (Z phase) of A, as PAIRS of neighbouring elements: the packed FMAs below take
      // one half of a pair as a broadcast operand (op_sel), so no {a, a} copies live in registers (the compiler's own splats cost 48
      // more registers and pushed the kernel to 2 waves per SIMD)
      f32x2v at0[8], at1[8], az[8];
      asm volatile("" ::: "memory");        // keeps these LDS reads (and their 48 registers) inside this branch
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        at0[i] = f32x2v{As[2 * (lane >> 4)][2 * i], As[2 * (lane >> 4)][2 * i + 1]};
        at1[i] = f32x2v{As[2 * (lane >> 4) + 1][2 * i], As[2 * (lane >> 4) + 1][2 * i + 1]};
        az[i] = f32x2v{As[lane & 7][2 * i], As[lane & 7][2 * i + 1]};
      }
      // (loaded per image visit, ~24 LDS reads against >= 20 items of work: kept out of the other modes' register budget)
      const int blk = lane >> 4, row = (lane >> 1) & 7, half = lane & 1;
      // LDS-DMA of item jq into a ring slot: the 2x4 input blocks of its two units are two runs of 512 contiguous bytes; lane l
      // moves 16-byte piece (l & 31) of run (l >> 5).  Branch-free (every iteration issues exactly one DMA and two stores, so the
      // hand-counted s_waitcnt below is exact): an index past j1 re-reads item j1 - 1 into a slot nobody consumes, and the
      // zero chroma of a grayscale JPEG (datasets.py:291-293) is a select on data DMA'd from a valid luma address.
      // Item cursors instead of a decode per item (round 6; tools/aug_prof.py: the loop ran ~330 instructions per item for its 48
      // FMAs, 200 of them scalar -- two unit_decode()s with their constant divisions, the source and destination addresses from
      // scratch, eight branches around a grayscale image's zero chroma).  Now the item being fetched (dc: RD - 1 items ahead,
      // parked on the visit's last item) and the item being computed (cc) are cursors that step by two units: a source pointer and
      // a destination offset in SGPRs that move by constants and are rebuilt only at a row / plane change; the per-lane part of
      // every address is a 32-bit register (scalar-base addressing), fixed per plane.
      typedef const char __attribute__((address_space(1)))* gchar_p;
      typedef short __attribute__((address_space(1)))* gshort_w;
      auto sgpr64 = [](unsigned long long v) {      // wave-uniform values that arrive in vector registers (yoff[b], coff[b], ...)
        const unsigned lo32 = __builtin_amdgcn_readfirstlane((unsigned)v), hi32 = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return ((unsigned long long)hi32 << 32) | lo32;
      };
      const unsigned long long srcY = sgpr64((unsigned long long)baseY), srcC = sgpr64((unsigned long long)baseC);
      const unsigned long long planeC_b = sgpr64((unsigned long long)planeC * 2);
      struct { int pl, oy, ox, S; unsigned long long p, prow; unsigned rstride, cstride; } dc;     // fetch cursor
      unsigned dloff = 0;                             // lane l moves 16-byte piece (l & 31) of input block row (l >> 5) of the item
      auto d_plane = [&]() {                          // (re)build the fetch cursor for plane dc.pl at (dc.oy, dc.ox)
        const bool zero = dc.pl && !a.has_chroma;     // grayscale: every chroma item re-reads luma block (0, 0) and is zeroed below
        const int plr = zero ? 0 : dc.pl;
        const int top = plr ? topC : topY, left = plr ? leftC : leftY, W = plr ? WC : WY;
        dc.S = dc.pl ? S_C : S_Y;
        dc.rstride = zero ? 0u : (unsigned)(2 * W * 128);
        dc.cstride = zero ? 0u : 512u;
        const unsigned long long base = plr ? srcC + (unsigned long long)(plr - 1) * planeC_b : srcY;
        dc.prow = base + ((unsigned long long)(unsigned)(top + (zero ? 0 : 2 * dc.oy)) * (unsigned)W + (unsigned)left) * 128ull;
        dc.p = dc.prow + (unsigned long long)(zero ? 0 : dc.ox) * 256ull;
        dloff = (unsigned)((lane >> 5) * W * 128 + (lane & 31) * 16);
      };
      // (a wave whose share starts behind the image's last item start has j0 == j1: its run-ahead DMAs still go out -- the
      // branch-free counting -- and must read a VALID item, so the cursors start at min(j0, j1 - 1); j1 >= 1 on every visit)
      int dj = min(j0, j1 - 1);
      unit_decode(2 * dj, dc.pl, dc.oy, dc.ox);
      struct { int pl, oy, ox, S; int orow, ocol; } cc;                                          // compute cursor
      cc.pl = dc.pl; cc.oy = dc.oy; cc.ox = dc.ox;
      d_plane();
      auto dma = [&](int slot) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((gchar_p)dc.p + dloff),
                                         (__attribute__((address_space(3))) void*)(ring + slot * 1024), 16, 0, 0);
        if (dj + 1 < j1) {
          ++dj;
          dc.ox += 2; dc.p += dc.cstride;
          if (dc.ox >= dc.S) {
            dc.ox = 0; dc.prow += dc.rstride; dc.p = dc.prow;
            if (++dc.oy >= dc.S) { dc.oy = 0; ++dc.pl; d_plane(); }
          }
        }
      };
      // quantisation rows of the three planes, read ONCE per image visit and before any DMA (vmcnt retires in order)
      short4v qv_y = *reinterpret_cast<const short4v*>(q + row * 8 + half * 4);            // (named scalars: an array indexed by
      short4v qv_b = *reinterpret_cast<const short4v*>(q + 64 + row * 8 + half * 4);       //  the plane ends up in scratch memory)
      short4v qv_r = *reinterpret_cast<const short4v*>(q + 128 + row * 8 + half * 4);
      {   // consumed HERE, in front of the first DMA: with table loads and LDS-DMAs pending together the compiler's wait for the
          // table is s_waitcnt vmcnt(0), i.e. a drain of the freshly started ring
        unsigned long long k0 = __builtin_bit_cast(unsigned long long, qv_y), k1 = __builtin_bit_cast(unsigned long long, qv_b),
                           k2 = __builtin_bit_cast(unsigned long long, qv_r);
        asm volatile("" : "+v"(k0), "+v"(k1), "+v"(k2));
        qv_y = __builtin_bit_cast(short4v, k0); qv_b = __builtin_bit_cast(short4v, k1); qv_r = __builtin_bit_cast(short4v, k2);
      }
#pragma unroll
      for (int t = 0; t < RD - 1; ++t) dma(t);
      const unsigned roff = (unsigned)((blk >> 1) * 512 + (blk & 1) * 128 + row * 16 + half * 8);   // unit A's 8 bytes in a slot; unit B: + 256
      const gshort_w img_g = (gshort_w)sgpr64((unsigned long long)img);
      // clamp bounds as operands instead of selects: no clamp = the int16 range
      const float dq_lo = a.raw ? -32768.f : (float)CMIN, dq_hi = a.raw ? 32767.f : (float)CMAX;
      const int out_lo = a.clamp_out ? CMIN : -32768, out_hi = a.clamp_out ? CMAX : 32767;
      const int negm = (flip && (lane & 1)) ? -1 : 0;             // int16 negation of the odd columns: (x ^ m) - m, wrapped below
      short4v qv = {0, 0, 0, 0};
      auto c_plane = [&]() {                                      // (re)build the compute cursor for plane cc.pl at (cc.oy, cc.ox)
        cc.S = cc.pl ? S_C : S_Y;
        cc.orow = (cc.pl == 0 ? 0 : NY + (cc.pl - 1) * NC1) + cc.oy * cc.S * 64;
        cc.ocol = (flip ? cc.S - 1 - cc.ox : cc.ox) * 64;
        const bool zero = cc.pl && !a.has_chroma;                 // zero chroma = zero quantisation factors (0 . c = 0, clamped 0)
        qv = cc.pl == 0 ? qv_y : (cc.pl == 1 ? qv_b : qv_r);
        if (zero) qv = short4v{0, 0, 0, 0};
      };
      c_plane();
      const int ostep = flip ? -128 : 128, onext = flip ? -64 : 64;
      for (int j = j0; j < j1; ++j) {
        const int t = j - j0;
        dma((t + RD - 1) % RD);
        // item j's DMA must have landed; younger operations that may stay in flight: the DMAs of j + 1 .. j + RD - 1 and the two
        // stores of each earlier iteration since it was issued  (3 RD - 3 in the steady state, RD - 1 + 2 t during start-up)
        static_assert(RD == 4, "wait counts below are written for RD = 4");
        if (__builtin_expect(t >= 3, 1)) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
        else if (t == 2) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
        else if (t == 1) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        // (read by inline asm: for an ordinary LDS load the compiler, which cannot see the counted wait above, inserts its own
        // s_waitcnt vmcnt(0) in front of any read of memory an LDS-DMA may have written -- and drains the whole ring)
        unsigned long long wA, wB;
        asm volatile("ds_read_b64 %0, %2\n\tds_read_b64 %1, %2 offset:256\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(wA), "=&v"(wB) : "v"(ring_lds + (unsigned)((t % RD) * 1024) + roff) : "memory");
        const short4v rA = __builtin_bit_cast(short4v, wA), rB = __builtin_bit_cast(short4v, wB);
        {
          float* xp = xt + ((blk & 1) * 8 + half * 4) * XP + ((blk >> 1) * 8 + row) * 2;     // Xt2[c][r][unit]
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const short cA = (short)((int)rA[e] * (int)qv[e]), cB = (short)((int)rB[e] * (int)qv[e]);    // int16 multiply WITH wrap-around (datasets.py:288)
            // the clamp on the converted value (integers: exact): one v_med3_f32 against bounds in registers
            *reinterpret_cast<f32x2v*>(xp + e * XP) = f32x2v{__builtin_amdgcn_fmed3f((float)cA, dq_lo, dq_hi), __builtin_amdgcn_fmed3f((float)cB, dq_lo, dq_hi)};
          }
        }
        __builtin_amdgcn_wave_barrier();
        {   // T = A[0:8,:] . X   (8 x 16): lane = (rows 2 ug, 2 ug + 1; column jj), both units
          const int jj = lane & 15, ug = lane >> 4;
          f32x2v t0 = {0.f, 0.f}, t1 = {0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < 8; ++kk) {
            const f32x4 v4 = *reinterpret_cast<const f32x4*>(xt + jj * XP + 4 * kk);    // {xA[2kk], xB[2kk], xA[2kk+1], xB[2kk+1]}
            const f32x2v x0 = {v4[0], v4[1]}, x1 = {v4[2], v4[3]};
            t0 = pk_fma_lo(at0[kk], x0, t0);
            t1 = pk_fma_lo(at1[kk], x0, t1);
            t0 = pk_fma_hi(at0[kk], x1, t0);
            t1 = pk_fma_hi(at1[kk], x1, t1);
          }
          *reinterpret_cast<f32x2v*>(tt + (2 * ug) * XP + jj * 2) = t0;
          *reinterpret_cast<f32x2v*>(tt + (2 * ug + 1) * XP + jj * 2) = t1;
        }
        __builtin_amdgcn_wave_barrier();
        const int u = lane >> 3;
        f32x2v z = {0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const f32x4 t4 = *reinterpret_cast<const f32x4*>(tt + u * XP + 4 * kk);
          z = pk_fma_lo(az[kk], f32x2v{t4[0], t4[1]}, z);
          z = pk_fma_hi(az[kk], f32x2v{t4[2], t4[3]}, z);
        }
        z = z / 2.0f;                                   // / sqrt(L*M)  (dct_ops.py:526)
        int vA = __float2int_rn(z[0]), vB = __float2int_rn(z[1]);   // torch.round = half-to-even, then int16 (dct_ops.py:578)
        vA = (int)(short)vA; vB = (int)(short)vB;
        vA = (int)(short)((vA ^ negm) - negm); vB = (int)(short)((vB ^ negm) - negm);     // flip: int16 negation, as the reference's tensors
        vA = vA < out_lo ? out_lo : (vA > out_hi ? out_hi : vA);
        vB = vB < out_lo ? out_lo : (vB > out_hi ? out_hi : vB);
        const gshort_w po = img_g + (cc.orow + cc.ocol);          // wave-uniform
        po[(unsigned)lane] = (short)vA;
        (po + onext)[(unsigned)lane] = (short)vB;
        cc.ox += 2; cc.ocol += ostep;
        if (cc.ox >= cc.S) {
          cc.ox = 0;
          if (++cc.oy >= cc.S) { cc.oy = 0; ++cc.pl; }
          c_plane();
        }
        __builtin_amdgcn_wave_barrier();
      }
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");     // the run-ahead DMAs have landed before anybody re-uses the ring (the last two stores may fly)
    } else if (mode == 1) {
      // ---- identity: item = eight consecutive output blocks, one 16-byte row per lane (de-quantise, clamp, flip), through the
      // same DMA ring: one DMA and one store per iteration, branch-free as above.
      const int u = lane & 7;
      auto dma = [&](int jq, int slot) {
        int pl, oy, ox;
        unit_decode(8 * min(jq, j1 - 1) + (lane >> 3), pl, oy, ox);
        const bool zero = pl && !a.has_chroma;      // grayscale JPEG: zero chroma (datasets.py:291-293)
        const int plr = zero ? 0 : pl, ry = zero ? 0 : oy, rx = zero ? 0 : ox;
        const int top = plr ? topC : topY, left = plr ? leftC : leftY, W = plr ? WC : WY;
        gshort_p src = plr ? baseC + (size_t)(plr - 1) * planeC : baseY;
        src += ((size_t)(top + ry) * W + left + rx) * 64 + u * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(ring + slot * 1024), 16, 0, 0);
      };
      short8v q8_y = *reinterpret_cast<const short8v*>(q + u * 8);            // quantisation rows, consumed before any DMA (see the /2 branch)
      short8v q8_b = *reinterpret_cast<const short8v*>(q + 64 + u * 8);
      short8v q8_r = *reinterpret_cast<const short8v*>(q + 128 + u * 8);
      asm volatile("" : "+v"(q8_y), "+v"(q8_b), "+v"(q8_r));
#pragma unroll
      for (int t = 0; t < RD - 1; ++t) dma(j0 + t, t);
      for (int j = j0; j < j1; ++j) {
        const int t = j - j0;
        dma(j + RD - 1, (t + RD - 1) % RD);
        // younger than item j's DMA: RD - 1 DMAs and one store per earlier iteration (2 RD - 2 steady, RD - 1 + t at start-up)
        if (t == 0) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else if (t == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (t == 2) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        short8v raw8;       // inline asm read: see the /2 branch
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(raw8) : "v"(ring_lds + (unsigned)((t % RD) * 1024 + lane * 16)) : "memory");
        int pl, oy, ox;
        unit_decode(8 * j + (lane >> 3), pl, oy, ox);
        const int S = pl ? S_C : S_Y;
        const bool zero = pl && !a.has_chroma;
        const short8v q8 = pl == 0 ? q8_y : (pl == 1 ? q8_b : q8_r);
        short8v val;
#pragma unroll
        for (int e = 0; e < 8; ++e) val[e] = zero ? (short)0 : dequant(raw8[e], q8[e], a.raw);
        if (flip) { val[1] = (short)-val[1]; val[3] = (short)-val[3]; val[5] = (short)-val[5]; val[7] = (short)-val[7]; }
        if (a.clamp_out) {
#pragma unroll
          for (int e = 0; e < 8; ++e) val[e] = clamp_s(val[e]);
        }
        *reinterpret_cast<short8v*>(img + (pl == 0 ? 0 : NY + (pl - 1) * NC1) + (oy * S + (flip ? S - 1 - ox : ox)) * 64 + u * 8) = val;
      }
      asm volatile("s_waitcnt vmcnt(1)" ::: "memory");     // run-ahead DMAs landed (see the /2 branch)
    } else {
      // ---- x2: item = one INPUT block -> 2x2 output blocks (dct_ops.py:474-482)
      float (*Xs)[17] = reinterpret_cast<float (*)[17]>(xt);
      float (*Ts)[17] = reinterpret_cast<float (*)[17]>(tt);
      constexpr int SYI = S_Y / 2, SCI = S_C / 2;
      auto src2 = [&](int j) -> gshort_p {
        int pl, iy, ix;
        if (j < SYI * SYI) { pl = 0; iy = j / SYI; ix = j % SYI; }
        else { const int u2 = j - SYI * SYI; pl = 1 + u2 / (SCI * SCI); iy = (u2 % (SCI * SCI)) / SCI; ix = u2 % SCI; }
        if (pl && !a.has_chroma) return nullptr;
        const int top = pl ? topC : topY, left = pl ? leftC : leftY, W = pl ? WC : WY;
        gshort_p src = pl ? baseC + (size_t)(pl - 1) * planeC : baseY;
        return src + ((size_t)(top + iy) * W + left + ix) * 64 + lane;
      };
      const short qx_y = q[lane], qx_b = q[64 + lane], qx_r = q[128 + lane];   // quantisation entries, before any prefetch (see the /2 branch)
      short nraw = 0;
      if (j0 < j1) { gshort_p sp = src2(j0); if (sp) nraw = *sp; }
      for (int j = j0; j < j1; ++j) {
        int pl, iy, ix, S;
        if (j < SYI * SYI) { pl = 0; S = S_Y; iy = j / SYI; ix = j % SYI; }
        else { const int u2 = j - SYI * SYI; pl = 1 + u2 / (SCI * SCI); S = S_C; iy = (u2 % (SCI * SCI)) / SCI; ix = u2 % SCI; }
        const bool zero = pl && !a.has_chroma;
        short* base = img + (pl == 0 ? 0 : NY + (pl - 1) * NC1);
        const short raw = nraw;
        if (j + 1 < j1) { gshort_p sp = src2(j + 1); if (sp) nraw = *sp; }
        {
          short val = 0;
          if (!zero) val = dequant(raw, pl == 0 ? qx_y : (pl == 1 ? qx_b : qx_r), a.raw);
          Xs[lane >> 3][lane & 7] = (float)val * 2.0f;            // * sqrt(L*M)
        }
        __builtin_amdgcn_wave_barrier();
        // T = A^T[:, 0:8] . P   (16 x 8):  T[r][j] = sum_{i<8} A[i][r] * P[i][j]
        {
          const int r = lane >> 2, c0 = (lane & 3) * 2;
          float t0 = 0.f, t1 = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float av = As[i][r];
            t0 = fmaf(av, Xs[i][c0], t0);
            t1 = fmaf(av, Xs[i][c0 + 1], t1);
          }
          Ts[r][c0] = t0;
          Ts[r][c0 + 1] = t1;
        }
        __builtin_amdgcn_wave_barrier();
        {
          const int r = lane >> 2, s0 = (lane & 3) * 4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int s = s0 + e;
            float y = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) y = fmaf(Ts[r][c], As[c][s], y);
            int val = (int)(short)__float2int_rn(y);
            const int oy = 2 * iy + (r >> 3), ox = 2 * ix + (s >> 3), kv = s & 7;
            const int oxf = flip ? S - 1 - ox : ox;
            if (flip && (kv & 1)) val = (int)(short)-val;
            if (a.clamp_out) val = clamp_s(val);
            base[(oy * S + oxf) * 64 + (r & 7) * 8 + kv] = (short)val;
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
#ifdef AUG_PROF
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    { const unsigned long long d = __builtin_readcyclecounter() - pf_m0; if (mode == 0) pf_c0 += d; else if (mode == 1) pf_c1 += d; else pf_c2 += d; }
#endif
  }
#ifdef AUG_PROF
  if (lane == 0 && wave < 4096) {
    unsigned long long* o = g_aug_prof + wave * 8;
    o[0] = pf_t0; o[1] = pf_t1; o[2] = __builtin_readcyclecounter();
    o[3] = ((unsigned long long)pf_n0 << 40) | ((unsigned long long)pf_n1 << 20) | (unsigned long long)pf_n2;
    o[4] = pf_c0; o[5] = pf_c1; o[6] = pf_c2;
    o[7] = ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) << 32) | __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));
  }
#endif
}

// ------------------------------------------------------------------------------------------------ kernel 2
// One 1024-thread workgroup per image; the working image (75 264 coefficients, 147 KB) lives in LDS for the whole op chain and
// every pass moves it as 16-byte ROWS (row u of one 8x8 block = 8 coefficients): 9 408 rows, 9.2 per thread.  Whole-block
// geometry (Translate, Rotate90) is staged through registers -- every thread gathers its destination rows from the LDS image,
// barrier, writes them back -- so nothing is spilled to global memory (the spill of the first version was the x1.46 write
// amplification of this kernel: 0.43 geometric ops per image x 150 KB).  S = 32: the image does not fit LDS and stays in its
// L2-resident slot of the intermediate buffer; same code through the same pointer (workgroup barriers order the workgroup's own
// global stores and loads on one CU).
constexpr int AUG_THREADS = 1024;
constexpr int NROWS = NIMG / 8;                                  // 16-byte rows per image
constexpr int ROWS_PT = (NROWS + AUG_THREADS - 1) / AUG_THREADS;  // 10 (S = 28) / 12 (S = 32)

struct RowPos { int pl, r, c, S, base; };        // plane, block row / column, plane side, element offset of the plane
__device__ __forceinline__ RowPos row_decode(int blkg) {          // blkg: block number in [Y | Cb | Cr] order (constant divisors)
  RowPos d;
  if (blkg < S_Y * S_Y) { d.pl = 0; d.S = S_Y; d.base = 0; d.r = blkg / S_Y; d.c = blkg % S_Y; }
  else {
    const int o = blkg - S_Y * S_Y;
    d.pl = 1 + o / (S_C * S_C); d.S = S_C; d.base = NY + (d.pl - 1) * NC1;
    const int o2 = o % (S_C * S_C);
    d.r = o2 / S_C; d.c = o2 % S_C;
  }
  return d;
}

__device__ __forceinline__ float linspace_f32(float start, float end, int steps, int i) {
  // torch.linspace fp32 CPU kernel: symmetric evaluation around the midpoint
  const float step = (end - start) / (float)(steps - 1);
  return i < steps / 2 ? start + step * (float)i : end - step * (float)(steps - 1 - i);
}

__device__ __forceinline__ short8v clamp8(short8v v) {          // four v_pk_max_i16 + four v_pk_min_i16
  const short8v lo = {CMIN, CMIN, CMIN, CMIN, CMIN, CMIN, CMIN, CMIN}, hi = {CMAX, CMAX, CMAX, CMAX, CMAX, CMAX, CMAX, CMAX};
  return __builtin_elementwise_min(__builtin_elementwise_max(v, lo), hi);
}
__device__ __forceinline__ void clamp_image(short* img, int tid, int nthreads) {
  short8v* p = reinterpret_cast<short8v*>(img);
  for (int i = tid; i < NROWS; i += nthreads) p[i] = clamp8(p[i]);
}

// Where kernel 2 reads an image's op records from: the two slots inside its rgbnm_aug_params (the three rgbnm_dct_augment* entries),
// or nops consecutive rgbnm_aug_op records (rgbnm_dct_augment_chain with an ops array, nops <= RGBNM_AUG_MAX_OPS).  Overloads on the
// pointer type: the kernel's text is the same for both, and each instantiation reads its records straight from memory.
struct OpRec { int op; float fm; int i0, i1, i2; };
__device__ __forceinline__ const rgbnm_aug_params* image_ops(const rgbnm_aug_params* prm, int b, int) { return prm + b; }
__device__ __forceinline__ const rgbnm_aug_op* image_ops(const rgbnm_aug_op* ops, int b, int nops) { return ops + (size_t)b * nops; }
__device__ __forceinline__ OpRec op_rec(const rgbnm_aug_params* pp, int slot) {
  return OpRec{pp->op[slot], pp->fmag[slot], pp->iarg0[slot], pp->iarg1[slot], pp->iarg2[slot]};
}
__device__ __forceinline__ OpRec op_rec(const rgbnm_aug_op* pp, int slot) {
  return OpRec{pp[slot].op, pp[slot].fmag, pp[slot].iarg0, pp[slot].iarg1, pp[slot].iarg2};
}

template <typename TO, typename REC>
__global__ __launch_bounds__(AUG_THREADS) void dct_randaug_kernel(short* inter, const REC* __restrict__ prm,
                                                                  const float* __restrict__ filt, TO* __restrict__ outY,
                                                                  TO* __restrict__ outC, int clamped, int nops) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr size_t IMG_LDS = IMG_IN_LDS ? NIMG * sizeof(short) : 0;
  const int b = blockIdx.x, tid = threadIdx.x;
  short* img = IMG_IN_LDS ? reinterpret_cast<short*>(smem_raw) : inter + (size_t)b * NIMG;
  short8v* rows = reinterpret_cast<short8v*>(img);
  int* red = reinterpret_cast<int*>(smem_raw + IMG_LDS);               // [48]
  unsigned char* smask = smem_raw + IMG_LDS + 256;                     // [S_Y * S_Y] Solarize: luma blocks to invert
  // block number -> (plane, block row, block column), decoded ONCE per workgroup (the constant divisions of row_decode() were a
  // third of the instructions of the row-wise passes: 10 rows per thread and op)
  unsigned* dtab = reinterpret_cast<unsigned*>(smem_raw + IMG_LDS + 256 + 1024);     // [UNITS]
  for (int blk = tid; blk < UNITS; blk += AUG_THREADS) {
    const RowPos d = row_decode(blk);
    dtab[blk] = (unsigned)d.pl | ((unsigned)d.r << 2) | ((unsigned)d.c << 8);
  }
  auto row_lookup = [&](int blk) {
    const unsigned w = dtab[blk];
    RowPos d;
    d.pl = (int)(w & 3u); d.r = (int)((w >> 2) & 63u); d.c = (int)(w >> 8);
    d.S = d.pl ? S_C : S_Y; d.base = d.pl == 0 ? 0 : NY + (d.pl - 1) * NC1;
    return d;
  };
  const REC* pp = image_ops(prm, b, nops);   // indexed per slot straight from memory (a local copy would go to scratch)
#ifdef AUG_PROF
  const unsigned long long pr0 = __builtin_readcyclecounter();
  unsigned long long pr1 = pr0, pr2 = pr0, pr3 = pr0;
#endif
  if (IMG_IN_LDS) {       // the entry clamp (custom_transforms.py:1106-1108) was applied by kernel 1's store: plain copy, all loads in flight
    const short8v* src = reinterpret_cast<const short8v*>(inter + (size_t)b * NIMG);
    short8v st[ROWS_PT];
#pragma unroll
    for (int k = 0; k < ROWS_PT; ++k) {
      const int i = tid + k * AUG_THREADS;
      if (i < NROWS) st[k] = src[i];
    }
#pragma unroll
    for (int k = 0; k < ROWS_PT; ++k) {
      const int i = tid + k * AUG_THREADS;
      if (i < NROWS) rows[i] = st[k];
    }
  }
  __syncthreads();
#ifdef AUG_PROF
  pr1 = __builtin_readcyclecounter();
#endif

  for (int slot = 0; slot < nops; ++slot) {
#ifdef AUG_PROF
    if (slot == 1) pr2 = __builtin_readcyclecounter();
#endif
    const OpRec rec = op_rec(pp, slot);
    const int op = rec.op;
    const float fm = rec.fm;
    const int i0 = rec.i0, i1 = rec.i1, i2 = rec.i2;
    if (op == RGBNM_OP_ROTATE90 || op == RGBNM_OP_TRANSLATEX || op == RGBNM_OP_TRANSLATEY) {
      // whole-block permutations (dct_ops.py:99-130, 748-774), in place: gather every destination row into registers, barrier, store.
      // Branch-free gathers (a row past the end re-reads the last row and is not stored), so that the LDS reads of all of a
      // thread's rows are in flight together: with a branch per row every row paid its own LDS round trips (tools/aug_prof.py).
      short8v st[ROWS_PT];
      if (op == RGBNM_OP_ROTATE90) {
        // per-block transpose: dst[u][v] = src[v][u].  The eight blocks of a wave lie a whole plane row apart in the source (a
        // multiple of 256 bytes: the same banks), so block j of the wave reads its elements in the order (e + j) & 7 -- eight
        // different 16-byte slots per instruction -- and the vector is rotated back by j places in registers.
        const int jsk = (tid >> 3) & 7;
#pragma unroll
        for (int k = 0; k < ROWS_PT; ++k) {
          const int i = min(tid + k * AUG_THREADS, NROWS - 1);
          const RowPos d = row_lookup(i >> 3);
          const int u = i & 7;
          int sr, sc;
          if (i0 > 0) { sr = d.c; sc = d.S - 1 - d.r; }        // counter-clockwise
          else { sr = d.S - 1 - d.c; sc = d.r; }               // clockwise
          const short* sp = img + d.base + ((sr * d.S + sc) << 6) + u;
#pragma unroll
          for (int e = 0; e < 8; ++e) st[k][e] = sp[((e + jsk) & 7) * 8];
        }
#pragma unroll
        for (int k = 0; k < ROWS_PT; ++k) {
          typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
          u32x4v q = __builtin_bit_cast(u32x4v, st[k]);           // out[e] = st[(e - j) & 7]
          if (jsk & 4) q = u32x4v{q[2], q[3], q[0], q[1]};
          if (jsk & 2) q = u32x4v{q[3], q[0], q[1], q[2]};
          if (jsk & 1) q = u32x4v{__builtin_amdgcn_alignbit(q[0], q[3], 16), __builtin_amdgcn_alignbit(q[1], q[0], 16),
                                  __builtin_amdgcn_alignbit(q[2], q[1], 16), __builtin_amdgcn_alignbit(q[3], q[2], 16)};
          short8v v = __builtin_bit_cast(short8v, q);
          const short8v nv = -v;                                   // int16 negation (wraps like the reference's tensors)
          if (i0 > 0) { if (tid & 1) v = nv; }                     // counter-clockwise: odd rows negated   (u = tid & 7 for every k)
          else v = short8v{v[0], nv[1], v[2], nv[3], v[4], nv[5], v[6], nv[7]};      // clockwise: odd columns negated
          st[k] = clamp8(v);                                       // - (-1024 .. -1017) leaves the range
        }
      } else {
        const int shY = i0, shC = i0 >= 0 ? i0 / 2 : -((-i0 + 1) / 2);               // python floor division //2
#pragma unroll
        for (int k = 0; k < ROWS_PT; ++k) {
          const int i = min(tid + k * AUG_THREADS, NROWS - 1);
          const RowPos d = row_lookup(i >> 3);
          const int sh = d.pl ? shC : shY;
          int sr = d.r, sc = d.c;
          if (op == RGBNM_OP_TRANSLATEX) sc -= sh;
          else sr -= sh;
          const bool in = sr >= 0 && sr < d.S && sc >= 0 && sc < d.S;
          const short8v v = *reinterpret_cast<const short8v*>(img + d.base + (((in ? sr : d.r) * d.S + (in ? sc : d.c)) << 6) + (i & 7) * 8);
          st[k] = in ? v : short8v{0, 0, 0, 0, 0, 0, 0, 0};        // moved as it is (clamped already, or the full pass below)
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < ROWS_PT; ++k) {
        const int i = tid + k * AUG_THREADS;
        if (i < NROWS) rows[i] = st[k];
      }
    } else if (op == RGBNM_OP_GRAYSCALE || op == RGBNM_OP_CHROMADROP) {
      // zero rows only: what stays is either clamped already (the image entered clamped) or meets the full pass below
      const int r0 = op == RGBNM_OP_GRAYSCALE ? NY / 8 : (NY + (i0 ? 0 : NC1)) / 8;
      const int r1 = op == RGBNM_OP_GRAYSCALE ? NROWS : r0 + NC1 / 8;
      for (int i = r0 + tid; i < r1; i += AUG_THREADS) rows[i] = short8v{0, 0, 0, 0, 0, 0, 0, 0};
    } else if (op == RGBNM_OP_CUTOUT) {
      // rows mirrored exactly as dct_ops.py:796-806 does; i0 = pad (luma), i1/i2 = centre (h, w) in luma blocks.  The rectangle of
      // each plane is walked directly (zero rows only, see above): thread -> (block of the rectangle, row of the block)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        const int S = pl ? S_C : S_Y, base = pl == 0 ? 0 : NY + (pl - 1) * NC1;
        const int pad = pl ? i0 / 2 : i0, ch = pl ? i1 / 2 : i1, cw = pl ? i2 / 2 : i2;
        const int lower = max(0, ch - pad), upper = max(0, S - ch - pad);
        const int left = max(0, cw - pad), right = max(0, S - cw - pad);
        const int rh = S - lower - upper, rw = S - right - left;          // rows [upper, S - lower), columns [left, S - right)
        if (rh <= 0 || rw <= 0) continue;
        const float inv = 1.0f / (float)rw;
        for (int t = tid; t < rh * rw * 8; t += AUG_THREADS) {
          const int blk = t >> 3;
          int rr = (int)(((float)blk + 0.5f) * inv);                       // blk / rw for blk < 784 (exact: the error is far below 0.5 / rw)
          const int cc = blk - rr * rw;
          *reinterpret_cast<short8v*>(img + base + (((upper + rr) * S + left + cc) << 6) + (t & 7) * 8) = short8v{0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
    } else if (op == RGBNM_OP_MIDFREQAUG || op == RGBNM_OP_SHARPNESS) {
      // Y only: x * F[u][v] -> clamp (fp32) -> round -> int16   (dct_ops.py:739-746 / 702-708)
      const float* F = filt + (size_t)i0 * 64;
      for (int i = tid; i < NY / 8; i += AUG_THREADS) {
        const f32x4 f0 = *reinterpret_cast<const f32x4*>(F + (i & 7) * 8), f1 = *reinterpret_cast<const f32x4*>(F + (i & 7) * 8 + 4);
        short8v v = rows[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float x = (float)v[e] * (e < 4 ? f0[e & 3] : f1[e & 3]);
          x = fminf(fmaxf(x, (float)CMIN), (float)CMAX);
          v[e] = clamp_s(__float2int_rn(x));
        }
        rows[i] = v;
      }
    } else if (op == RGBNM_OP_EQUALIZE) {
      // equalize_dct on Y (dct_ops.py:916-955): new DC = round((cdf[dc] - cdf_min) / (N - cdf_min) * 2039) + CMIN with
      // cdf[v] = #{DC <= v}, cdf_min = #{DC == min}; fp32 divide and multiply, round half to even.  Rank counting
      // over the S*S luma DCs (each thread: one DC against all others, broadcast LDS / L2 reads) - exact integers.
      constexpr int N = S_Y * S_Y;
      int mine = 0, le = 0, mn = 32767;
      if (tid < N) mine = img[tid * 64];
      for (int i = 0; i < N; ++i) {
        const int o = img[i * 64];
        le += (tid < N && o <= mine) ? 1 : 0;
        mn = min(mn, o);
      }
      int cmin = 0;
      for (int i = 0; i < N; ++i) cmin += img[i * 64] == mn ? 1 : 0;
      __syncthreads();                      // every thread has read the original DCs
      if (tid < N) {
        // a flat image (every DC equal, N - cmin == 0) divides 0 by 0 in the reference; its int16 cast makes 0 of the NaN and the
        // shift back gives CMIN for every DC, whatever the DC was (tests/golden/g24_flat.npz)
        const float eq = N - cmin > 0 ? rintf((float)(le - cmin) / (float)(N - cmin) * (float)(CMAX - CMIN - 1)) : 0.f;
        img[tid * 64] = clamp_s((int)eq + CMIN);
      }
    } else if (op == RGBNM_OP_INVERT || op == RGBNM_OP_SOLARIZE || op == RGBNM_OP_FREQENHANCE) {
      // whole-block ops outside the default lists (SURVEY 8f f4): invert_dct (dct_ops.py:623-629), solarize_dct (:631-651:
      // blocks whose ORIGINAL luma DC exceeds the threshold are negated; chroma block (r,c) follows luma block (2r,2c),
      // custom_transforms.py:981-983), freq_enhance_dct (:1015-1035: AC * factor, round half to even, DC untouched)
      if (op == RGBNM_OP_SOLARIZE) {
        for (int i = tid; i < S_Y * S_Y; i += AUG_THREADS) smask[i] = img[i * 64] > i0 ? 1 : 0;
        __syncthreads();
      }
      for (int i = tid; i < NROWS; i += AUG_THREADS) {
        const RowPos d = row_lookup(i >> 3);
        short8v v = rows[i];
        bool neg = op == RGBNM_OP_INVERT;
        if (op == RGBNM_OP_SOLARIZE) neg = (d.pl == 0 ? smask[d.r * S_Y + d.c] : smask[2 * d.r * S_Y + 2 * d.c]) != 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          int x = v[e];
          if (op == RGBNM_OP_FREQENHANCE) { if (e != 0 || (i & 7) != 0) x = __float2int_rn((float)x * fm); }
          else if (neg) x = (int)(short)-x;                       // int16 negation (wraps like the reference's tensors: only -32768, on an unclamped image)
          v[e] = clamp_s(x);
        }
        rows[i] = v;
      }
    } else if (op != RGBNM_OP_IDENTITY) {
      // ---- DC photometric ops: exact integer reduction over the DC set, fp32 update, round, clamp ----
      const bool onC = (op == RGBNM_OP_COLOR || op == RGBNM_OP_AUTOSATURATION);
      const bool both = (op == RGBNM_OP_POSTERIZE);
      const int ndc = onC ? 2 * S_C * S_C : S_Y * S_Y;
      const int dcbase = onC ? NY : 0;
      float gsum = 0.f, gmin = 0.f, gmax = 0.f;
      if (op == RGBNM_OP_BRIGHTNESS || op == RGBNM_OP_AUTOCONTRAST || op == RGBNM_OP_AUTOSATURATION) {
        int s = 0, mn = 32767, mx = -32768;
        for (int i = tid; i < ndc; i += AUG_THREADS) {
          const int dc = img[dcbase + i * 64];
          s += dc < 0 ? -dc : dc;
          mn = min(mn, dc);
          mx = max(mx, dc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          s += __shfl_xor(s, o, 64);
          mn = min(mn, __shfl_xor(mn, o, 64));
          mx = max(mx, __shfl_xor(mx, o, 64));
        }
        if ((tid & 63) == 0) { red[(tid >> 6) * 3] = s; red[(tid >> 6) * 3 + 1] = mn; red[(tid >> 6) * 3 + 2] = mx; }
        __syncthreads();
        s = 0; mn = 32767; mx = -32768;
        for (int wv = 0; wv < AUG_THREADS / 64; ++wv) { s += red[wv * 3]; mn = min(mn, red[wv * 3 + 1]); mx = max(mx, red[wv * 3 + 2]); }
        gsum = (float)s;               // |DC| <= 1024, <= 784 terms: exact in fp32 in any summation order
        gmin = (float)mn;
        gmax = (float)mx;
        __syncthreads();
      }
      const int total = both ? S_Y * S_Y + 2 * S_C * S_C : ndc;
      for (int i = tid; i < total; i += AUG_THREADS) {
        const int idx = both ? (i < S_Y * S_Y ? i * 64 : NY + (i - S_Y * S_Y) * 64) : dcbase + i * 64;
        const short dc16 = img[idx];
        float dc = (float)dc16;
        int res;
        if (op == RGBNM_OP_BRIGHTNESS) {
          dc = dc + (gsum / (float)ndc) * fm;                      // fm = factor - 1  (dct_ops.py:832)
          res = __float2int_rn(dc);
        } else if (op == RGBNM_OP_CONTRAST || op == RGBNM_OP_COLOR) {
          res = __float2int_rn(dc * fm);                           // fm = factor      (dct_ops.py:856)
        } else if (op == RGBNM_OP_AUTOCONTRAST || op == RGBNM_OP_AUTOSATURATION) {
          if (gmin == gmax && gmax == 0.f) res = dc16;             // dct_ops.py:879
          else {
            dc = (dc - gmin) / (gmax - gmin);
            dc = (float)CMIN + dc * (float)(CMAX - CMIN);
            res = __float2int_rn(dc);
          }
        } else if (op == RGBNM_OP_POSTERIZE) {
          dc = (dc - (float)CMIN) / (float)(1 << i0);              // i0 = bit offset
          const int k = __float2int_rn(dc);
          res = __float2int_rn(linspace_f32((float)CMIN, (float)CMAX, i1, k));   // i1 = table length
        } else {   // RGBNM_OP_SOLARIZEADD: int16 add below threshold 0 (dct_ops.py:672-677)
          res = dc16 < 0 ? (int)(short)(dc16 + (short)i0) : (int)dc16;
        }
        img[idx] = clamp_s((int)(short)res);
      }
    }
    __syncthreads();
    if (!clamped) {
      // per-op clamp (custom_transforms.py:1019-1020).  Every branch above clamps what it writes, so on an image that entered
      // clamped (kernel 1's store: the RandAugment entry clamp, :1106-1108) the reference's whole-tensor clamp after each op is
      // the identity on everything else.  Only an image that entered unclamped needs one full pass, after its first op.
      clamp_image(img, tid, AUG_THREADS);
      __syncthreads();
      clamped = 1;
    }
  }

#ifdef AUG_PROF
  pr3 = __builtin_readcyclecounter();
#endif
  // ---- ToRange (custom_transforms.py:451-452): ((x + 1024) / 2040) * 2 - 1, fp32, then cast ----
  TO* oy = outY + (size_t)b * NY;
  TO* oc = outC + (size_t)b * 2 * NC1;
  for (int e8 = tid * 8; e8 < NIMG; e8 += AUG_THREADS * 8) {      // NY % 8 == 0: a vector never straddles Y / CbCr
    const short8v c = *reinterpret_cast<const short8v*>(img + e8);
    TO* dst = e8 < NY ? oy + e8 : oc + (e8 - NY);
    if constexpr (__is_same(TO, short)) {
      // raw int16 output (out_dtype 2): the coefficients as they are, no ToRange -- what the per-transform classes of
      // custom_transforms.py hand to the next transform of a Compose chain
      *reinterpret_cast<short8v*>(dst) = c;
    } else {
      f32x4 v[2];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        // (x + 1024) / 2040 without the division sequence (11 instructions per coefficient: this loop was VALU-bound at 12 k
        // cycles per image): q0 = n R, one residual step.  Equal to the IEEE quotient for EVERY int16 x -- checked exhaustively
        // (tests/test_augment.py::test_torange_quotient_is_exact_for_every_int16).
        const float n = (float)c[k] - (float)CMIN;
        constexpr float R = 1.0f / (float)(CMAX - CMIN);
        const float q0 = n * R;
        const float x = __builtin_fmaf(__builtin_fmaf(-q0, (float)(CMAX - CMIN), n), R, q0);
        v[k >> 2][k & 3] = __builtin_fmaf(x, 2.0f, -1.0f);
      }
      if constexpr (__is_same(TO, bf16)) {
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (bf16)v[k >> 2][k & 3];
        *reinterpret_cast<bf16x8*>(dst) = o;
      } else if constexpr (__is_same(TO, f16)) {
        // the fp32 ToRange value rounded ONCE to IEEE half (round to nearest even: from_f32<f16> keeps the compiler from folding
        // the last fma into the conversion), eight coefficients per 16-byte store like bf16
        f16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = from_f32<f16>(v[k >> 2][k & 3]);
        *reinterpret_cast<f16x8*>(dst) = o;
      } else {
        store4<TO>(dst, v[0]);
        store4<TO>(dst + 4, v[1]);
      }
    }
  }
#ifdef AUG_PROF
  if ((tid & 63) == 0 && b < 256) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned long long* o = g_aug_prof2 + (b * 16 + (tid >> 6)) * 8;
    o[0] = pr0; o[1] = pr1; o[2] = pr2; o[3] = pr3; o[4] = __builtin_readcyclecounter(); o[5] = op_rec(pp, 0).op; o[6] = op_rec(pp, 1).op;
  }
#endif
}


inline size_t workspace_bytes(int B) { return (size_t)B * NIMG * sizeof(short); }

// workgroups of kernel 1 that are resident at once on this device (CUs x occupancy): the grid is exactly one round of them
inline int resize_grid() {
  static std::atomic<int> cached[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  dev &= 63;
  int g = cached[dev].load(std::memory_order_acquire);
  if (g > 0) return g;
  int cus = 256, occ = 4;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)dct_resize_kernel, 256, RESIZE_LDS) != hipSuccess || occ <= 0) occ = 4;
  g = cus * occ;
  cached[dev].store(g, std::memory_order_release);
  return g;
}

// kernel 2 for one output type and one source of the op records
template <typename TO, typename REC>
inline int launch_randaug(short* inter, const REC* recs, const float* filters, void* outY, void* outC, int B, int clamped, int nops,
                          size_t smem, hipStream_t st) {
  static DevOnce attr;
  if (attr.need()) {
    if (hipFuncSetAttribute((const void*)dct_randaug_kernel<TO, REC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return RGBNM_ELAUNCH;
    attr.done();
  }
  hipLaunchKernelGGL((dct_randaug_kernel<TO, REC>), dim3(B), dim3(AUG_THREADS), smem, st, inter, recs, filters, (TO*)outY, (TO*)outC,
                     clamped, nops);
  return RGBNM_OK;
}

// out_code: RGBNM_AUG_OUT_* (0 fp32, 1 bf16, 2 raw int16, 3 fp16; the three older entries refuse 3 before they get here).
// ops_dev / ops_host: [B][nops] rgbnm_aug_op records that replace the op fields of the parameters (rgbnm_dct_augment_chain), or null.
inline int launch(const int16_t* Yq, const int16_t* CbCrq, const int16_t* quant, const rgbnm_aug_params* params_dev,
                  const rgbnm_aug_params* params_host, const float* conv16, const float* filters, void* outY, void* outC,
                  int out_code, int B, int Hy, int Wy, int Hc, int Wc, int entry_clamp, int nops, void* workspace,
                  size_t ws_bytes, hipStream_t st, const long long* yoff = nullptr, const long long* coff = nullptr,
                  const rgbnm_aug_op* ops_dev = nullptr, const rgbnm_aug_op* ops_host = nullptr) {
  if (ws_bytes < workspace_bytes(B)) return RGBNM_EWORKSPACE;
  if ((yoff != nullptr) != (coff != nullptr)) return RGBNM_EINVAL;
  if (out_code < RGBNM_AUG_OUT_F32 || out_code > RGBNM_AUG_OUT_F16) return RGBNM_EINVAL;      // before kernel 1 goes out, not after it
  // host-side validation of every crop box (the HIP path implements the x2 / identity / /2 resize cases)
  for (int b = 0; b < B; ++b) {
    const rgbnm_aug_params& p = params_host[b];
    if (p.crop_h != p.crop_w) return RGBNM_EINVAL;
    if (p.crop_w != 2 * S_Y && p.crop_w != S_Y && 2 * p.crop_w != S_Y) return RGBNM_EINVAL;
    if ((p.crop_i & 1) || (p.crop_j & 1) || p.crop_i < 0 || p.crop_j < 0) return RGBNM_EINVAL;
    if (p.crop_i + p.crop_h > Hy || p.crop_j + p.crop_w > Wy) return RGBNM_EINVAL;
    if (CbCrq && (p.crop_i / 2 + p.crop_h / 2 > Hc || p.crop_j / 2 + p.crop_w / 2 > Wc)) return RGBNM_EINVAL;
    for (int s = 0; s < nops; ++s) {
      const int op = ops_host ? ops_host[(size_t)b * nops + s].op : p.op[s];
      if (op < 0 || op > RGBNM_OP_EQUALIZE) return RGBNM_EINVAL;
      // the only readers of `filters`: without a bank kernel 2 would read through the null pointer
      if (!filters && (op == RGBNM_OP_MIDFREQAUG || op == RGBNM_OP_SHARPNESS)) return RGBNM_EINVAL;
    }
  }
  // algorithmic bytes of the stage (SURVEY.md 8d): the crop box in (192 w^2 B for side w: luma w^2 blocks + 2 chroma planes of
  // (w/2)^2, 128 B each) + the quantisation tables, the S x S image out in its output type -- the int16 intermediate is not counted
  double abytes = 0.0;
  for (int b = 0; b < B; ++b) abytes += 192.0 * params_host[b].crop_w * params_host[b].crop_w + 384.0;
  abytes += (double)B * NIMG * (out_code == RGBNM_AUG_OUT_F32 ? 4.0 : 2.0);
  const int tslot = rgbnm_trace_begin(TR_AUG, 0.0, abytes, st);
  const int grid = resize_grid();
  for (int b0 = 0; b0 < B; b0 += RESIZE_MAXB) {          // the cost prefix table of one launch covers RESIZE_MAXB images
    const int nb = B - b0 < RESIZE_MAXB ? B - b0 : RESIZE_MAXB;
    ResizeArgs a;
    a.Yq = yoff ? Yq : Yq + (size_t)b0 * Hy * Wy * 64;          // packed: the offsets are absolute
    a.Cq = CbCrq ? (yoff ? CbCrq : CbCrq + (size_t)b0 * 2 * Hc * Wc * 64) : nullptr;
    a.yoff = yoff ? yoff + b0 : nullptr; a.coff = coff ? coff + b0 : nullptr;
    a.quant = quant + (size_t)b0 * 192; a.prm = params_dev + b0; a.A16 = conv16;
    a.img = (short*)workspace + (size_t)b0 * NIMG;
    a.B = nb; a.Hy = Hy; a.Wy = Wy; a.Hc = Hc; a.Wc = Wc; a.has_chroma = CbCrq != nullptr;
    a.raw = (entry_clamp >> 1) & 1;      // bit 1: input already de-quantised: no clamp in front of the crop / resize stage
    a.clamp_out = entry_clamp & 1;       // bit 0: RandAugment's entry clamp, applied by this kernel's store
    a.pfx[0] = 0;
    for (int b = 0; b < nb; ++b) a.pfx[b + 1] = a.pfx[b] + cost_of(mode_of(params_host[b0 + b].crop_w));
    hipLaunchKernelGGL(dct_resize_kernel, dim3(grid), dim3(256), RESIZE_LDS, st, a);
    LAUNCH_CHECK();
  }
  entry_clamp &= 1;
  short* inter = (short*)workspace;
  const size_t smem = (IMG_IN_LDS ? NIMG * sizeof(short) : 0) + 256 + 1024 + UNITS * 4;   // image + reduction scratch + Solarize mask + block decode table
  int rc;
#define AUG_K2(TO)                                                                                                               \
  (ops_dev ? launch_randaug<TO, rgbnm_aug_op>(inter, ops_dev, filters, outY, outC, B, entry_clamp, nops, smem, st)                \
           : launch_randaug<TO, rgbnm_aug_params>(inter, params_dev, filters, outY, outC, B, entry_clamp, nops, smem, st))
  if (out_code == RGBNM_AUG_OUT_F32) rc = AUG_K2(float);
  else if (out_code == RGBNM_AUG_OUT_BF16) rc = AUG_K2(bf16);
  else if (out_code == RGBNM_AUG_OUT_I16) rc = AUG_K2(short);          // raw int16 coefficients (no ToRange)
  else rc = AUG_K2(f16);
#undef AUG_K2
  if (rc != RGBNM_OK) return rc;
  rgbnm_trace_end(tslot, st);
  LAUNCH_CHECK();
  return RGBNM_OK;
}

}  // namespace AUG_NS
