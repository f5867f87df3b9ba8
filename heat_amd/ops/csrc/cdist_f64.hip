// hipcc-flags: -fno-slp-vectorize
// Native float64 pairwise distances (ha_cdist_f64, behind ops.cdist_f64): what float64 input of
// ht.spatial.cdist / rbf / manhattan, cdist_topk, KMedians and KMedoids runs on. Two tile kernels
// whose epilogue IS the distance, so the m x n fp64 matrix is written once and never re-read, and a
// row-norm pre-pass. Mode numbering of ha_cdist (cdist.hip); everything is double, 64-bit offsets.
//
// (a) cdist_f64_mm, modes 0-2: d2 = |x|^2 + |y|^2 - 2 x.y on v_mfma_f64_16x16x4_f64, then clamp at
//     0, then sqrt / nothing / exp(-scale d2), then the store.
//   * 128 x 128 outputs per 4-wave workgroup, each wave 64 x 64 = 4 x 4 accumulator blocks (128
//     registers per lane), two workgroups per CU so one tile's epilogue overlaps the other's MFMAs;
//   * both operands are k-contiguous ([rows][f]) and come through the 4-slot staging ring that
//     f64_ring.h describes (image, pipeline, tail). f here is 3 to a few
//     hundred, so the loop is written for short trip counts: fewer stages than the ring (down to
//     f = 1), f no multiple of 8 and odd f all run the same guarded steps;
//   * row norms come from f64_row_norms (f64_ring.h: bit-identical for a row wherever it sits),
//     m + n doubles of workspace read per tile in the epilogue; X == Y computes them once. The
//     pre-pass reads (m + n) f values against m n written: f (1 / m + 1 / n) of the store traffic,
//     below 1 % for the 40000 x 40000 shapes up to f = 200 and no longer negligible once
//     min(m, n) < ~10 f (a handful of medoids against many features);
//   * stores are non-temporal. Which operand feeds the MFMA's A side decides what a lane owns (the
//     f64 16x16x4 C/D map is column = lane & 15, row = (lane >> 4) + 4 g). X is on A: a lane owns
//     one column of 4 rows, 8-byte stores, 16 lanes = one 128-byte run, any alignment of C.
//     Measured alternative, not kept (profiles/cdist_f64_r08_store16.jsonl): Y on A with the A
//     fragment rows read permuted (lane r reads block row 4 (r & 3) + (r >> 2)), so a lane owns 4
//     CONSECUTIVE columns of one row and stores them as two 16-byte stores (4 lanes = one 128-byte
//     run, 16 rows per instruction) when C is 16-byte aligned with an even ldc: 40000 x 40000,
//     f = 18: 4.83 ms against 3.55 ms for the 8-byte form in the same run; f = 128: 8.16 against
//     8.21 ms; 2000 x 2000 x 18: 0.018 against 0.019 ms;
//   * out-of-range rows / columns are clamped at the load and masked at the store;
//   * 1-D grid in an XCD-aware grouped order: each XCD gets a contiguous run of tiles, in which 8
//     X tiles at a time sweep all Y tiles (8 consecutive workgroups share one Y tile).
//   Requirements (made so by the Python wrapper, never by a copy in here): the ring's, on X and Y.
//
// (b) cdist_f64_vx, modes 3-6: sum |x - y| or sum (x - y)^2 on the fp64 VALU, the only form without
//     cancellation for near-identical rows.
//   * 128 x 128 outputs per 256-thread workgroup, 8 x 8 per thread (64 fp64 accumulators): thread
//     (tr, tc) owns rows 2 tr + 32 i + {0, 1} and columns 2 tc + 32 j + {0, 1};
//   * chunks of 16 features staged transposed ([feature][row], row stride 130) so a thread reads two
//     of its rows per ds_read_b128 (16 lanes = 256 contiguous bytes, the x side a broadcast); all of
//     a chunk's global loads (plain 8-byte loads with clamped addresses: any row stride, any 8-byte
//     alignment, nothing read past column f of the last row) are issued before the previous chunk's
//     inner loop and written to the OTHER LDS buffer after it: one barrier per chunk, 65 KB per
//     workgroup, two workgroups per CU;
//   * per feature and pair: v_add_f64 (subtract) + v_fma_f64, manhattan v_add_f64 with |.|;
//   * every pair's sum runs over the features in index order 0 .. f - 1 whatever the tile or the
//     chunking, so d(i, j) depends neither on m, n, the tile position nor on how the rows are
//     split over ranks (cdist_topk's tie rule), and d(i, j) == d(j, i) bitwise;
//   * symmetric (bit 8: Y is X, m == n, same stride): only tiles on or above the diagonal are
//     launched and each off-diagonal tile is stored a second time mirrored, as cdist_vx<OP, true>;
//   * non-temporal stores of the thread's column pairs: 16 bytes (16 lanes = one 256-byte run) when
//     C is 16-byte aligned with an even ldc, else 8 bytes.
//
// Compile figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//   kernel                    VGPRs  AGPRs  SGPRs  LDS bytes  scratch  occupancy (waves / SIMD)
//   cdist_f64_mm<OP>           216      0     76     65536        0       2
//   cdist_f64_vx<OP, false>    242      0  47-56     66560        0       2
//   cdist_f64_vx<OP, true>     244      0  30-56     66560        0       2
//   f64_row_norms               12      0     20         0        0       8
// 2 waves per SIMD = two workgroups per CU for both tile kernels; the 8 x 8 fp64 VALU tile does not
// spill, so the 8 x 4 fallback was not needed.
//
// Measured (MI355X, tools/microbench/cdist_f64.py, profiles/cdist_f64_r08.jsonl; ms of 3 rounds,
// "before" = the torch expressions device float64 distances ran on, GB/s = output written):
//   40000 x 40000      f    native ms      GB/s   before ms
//   expansion eucl.   18    3.55 - 3.59    3600   22.4   (addmm, clamp, sqrt)
//   expansion eucl.  128    8.19 - 8.26    1560   25.7   (fp64 MFMA work: 50 TF)
//   exact eucl.       18    4.24 - 4.28    3000   (*)
//   exact eucl.      128   16.41 - 16.49    780   (*)
//   exact, symmetric 128    9.12 - 9.22    1400   (*)    1.79 x the full call
//   manhattan         18    3.19 - 3.28    3950   (*)
//   manhattan        128   14.50 - 14.73    880   (*)
//   2000 x 2000 x 18: expansion 0.019 (before 0.075), exact 0.016 (2.59), manhattan 0.014 (2.55)
// (*) torch.cdist's difference kernels (p = 1, and p = 2 without the matrix product) leave most of a
// 40000 x 40000 float64 result unwritten (errors of 11 - 198 against the broadcast expression on
// sampled rows, 13.1 - 13.5 ms and 4.1 - 4.4 ms whatever f), so there is no time of a complete result
// to compare with; the native results agree with the broadcast expression to 3e-13 there.
// Against the estimates this was planned with: the expansion tile writes 3.6 TB/s at f = 18 and is
// matrix-core-bound at f = 128 (50 TF of the 78 TF peak); the crossover between the two was not
// measured. The VALU kernel at f = 128 issues 2 f fp64 operations per pair at 25 T lane-operations
// per second (65 % of the VALU's fp64 issue rate); from where on in f it is compute-bound was not
// measured beyond these two points.
#include "f64_ring.h"

#include <cmath>

namespace {

// OP of both kernels' epilogue: what becomes of the summed value v (d2, or d1 for manhattan)
enum { OP_L1 = 0, OP_EUCLID = 1, OP_SQ = 2, OP_GAUSS = 3 };

template <int OP>
__device__ __forceinline__ double cf_fin(double v, double scale) {
  if (OP == OP_EUCLID) return sqrt(v);
  if (OP == OP_GAUSS) return exp(-scale * v);
  return v;
}

__device__ __forceinline__ void cf_store2(double* p, double a, double b) {
  __builtin_nontemporal_store((doublex2){a, b}, reinterpret_cast<doublex2*>(p));
}

// --------------------------------------------------------------------- (a) expansion on the MFMA
constexpr int CT = F64_T;          // tile rows / columns
constexpr int CNBUF = 4;           // ring slots
constexpr int CAHEAD = CNBUF - 1;  // stages in flight

// Fragments of one stage for a wave: p[b][s], q[b][s] = block b's operand for MFMA k-step s.
struct CfFrag {
  double p[4][2], q[4][2];
};

// X feeds the MFMA's A side ("P": the rows of the accumulator blocks), Y the B side ("Q").
template <int OP>
__global__ __launch_bounds__(256, 2) void cdist_f64_mm(const double* __restrict__ X, int64_t m,
                                                       const double* __restrict__ Y, int64_t n, int64_t f,
                                                       int64_t ldx, int64_t ldy, const double* __restrict__ xn,
                                                       const double* __restrict__ yn, double* __restrict__ C,
                                                       int64_t ldc, double scale) {
  static_assert(CNBUF * F64_STG <= 80 * 1024, "two workgroups per CU");
  __shared__ __attribute__((aligned(16))) unsigned char smem[CNBUF * F64_STG];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int kk = lane >> 4, r = lane & 15;
  const unsigned ty = (unsigned)((n + CT - 1) / CT), tx = (unsigned)((m + CT - 1) / CT);
  const unsigned bid = ha_xcd_remap(blockIdx.x, tx * ty);
  constexpr unsigned GM = 8;
  const unsigned grp = bid / (GM * ty), gfirst = grp * GM;
  const unsigned gsz = tx - gfirst < GM ? tx - gfirst : GM;
  const int64_t x0 = (int64_t)(gfirst + (bid % (GM * ty)) % gsz) * CT, y0 = (int64_t)((bid % (GM * ty)) / gsz) * CT;

  F64Src<> sp, sq;
  sp.init(X, ldx, m, x0, lane);
  sq.init(Y, ldy, n, y0, lane);
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

  auto stage = [&](int64_t t, bool full) {
    const unsigned dst = sbase + (unsigned)((t % CNBUF) * F64_STG);
    const int64_t k0 = t * F64_K;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      ha_dma16(full ? sp.src(k0, q) : sp.src_clamped(k0, q, f), dst + q * 1024);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      ha_dma16(full ? sq.src(k0, q) : sq.src_clamped(k0, q, f), dst + F64_OP + q * 1024);
    }
  };
  // this wave's own pieces of the tail stage: the values at k >= f become zero
  auto zero_tail = [&](int64_t t) {
    unsigned char* dst = smem + (t % CNBUF) * F64_STG;
    const int64_t ka = t * F64_K + 2 * wave;  // both of this wave's pieces hold the pair ka, ka + 1
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      double* pa = reinterpret_cast<double*>(dst + q * 1024 + lane * 16);
      double* pb = reinterpret_cast<double*>(dst + F64_OP + q * 1024 + lane * 16);
      if (ka >= f) pa[0] = pb[0] = 0.0;
      if (ka + 1 >= f) pa[1] = pb[1] = 0.0;
    }
  };

  // fragment reads: block bl of the wave's 64 rows from w0, lane's row r within the block
  auto opnd = [&](const unsigned char* b, int w0, double (*o)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int bl = 0; bl < 4; ++bl) {
      const doublex2 v = *reinterpret_cast<const doublex2*>(b + kk * (CT * 16) + (w0 + 16 * bl + r) * 16);
      o[bl][0] = v[0];
      o[bl][1] = v[1];
    }
  };
  auto load = [&](CfFrag& F, int64_t t) {
    const unsigned char* base = smem + (t % CNBUF) * F64_STG;
    opnd(base, wm * 64, F.p);
    opnd(base + F64_OP, wn * 64, F.q);
  };

  doublex4 acc[4][4];
#pragma unroll
  for (int bm = 0; bm < 4; ++bm)
#pragma unroll
    for (int bn = 0; bn < 4; ++bn) acc[bm][bn] = (doublex4)(0.0);

  // the stage's 32 MFMAs in two halves (block rows 0-1 / 2-3) around the barrier
  auto mma_half = [&](const CfFrag& F, int part) {
#pragma unroll
    for (int bm = 2 * part; bm < 2 * part + 2; ++bm)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int bn = 0; bn < 4; ++bn)
          acc[bm][bn] = __builtin_amdgcn_mfma_f64_16x16x4f64(F.p[bm][s], F.q[bn][s], acc[bm][bn], 0, 0, 0);
  };

  const int64_t nk = (f + F64_K - 1) / F64_K;
  const bool tail = (f % F64_K) != 0;
  // stage t landed (this wave's DMA) and visible to every wave; later stages may be in flight
  auto ready = [&](int64_t t) {
    const int64_t later = nk - 1 - t < CAHEAD - 1 ? nk - 1 - t : CAHEAD - 1;  // stages issued after t
    if (tail && t == nk - 1) {
      ha_vm_wait<0>();
      zero_tail(t);
    }
    if (later >= 2) ha_wait_barrier<2 * F64_DPS>();
    else if (later == 1) ha_wait_barrier<F64_DPS>();
    else ha_wait_barrier<0>();
  };
  // steady state (f >= 40): stage t + AHEAD issued whole, the first half of the MFMAs around it,
  // the counted wait for stage t + 1 + barrier, stage t + 1's fragment reads between the second
  // half's MFMAs
  auto step_full = [&](int64_t t, const CfFrag& Fc, CfFrag& Fn) {
    stage(t + CAHEAD, true);
    mma_half(Fc, 0);
    __builtin_amdgcn_sched_barrier(0);
    ha_wait_barrier<(CAHEAD - 1) * F64_DPS>();
    load(Fn, t + 1);
    mma_half(Fc, 1);
    __builtin_amdgcn_sched_barrier(0);
  };
  // the guarded step: the whole loop for f < 40, and the last stages otherwise
  auto step = [&](int64_t t, const CfFrag& Fc, CfFrag& Fn) {
    if (t + CAHEAD < nk) stage(t + CAHEAD, !(tail && t + CAHEAD == nk - 1));
    mma_half(Fc, 0);
    if (t + 1 < nk) {
      ready(t + 1);
      load(Fn, t + 1);
    }
    mma_half(Fc, 1);
  };

  CfFrag F0, F1;
  for (int64_t t = 0; t < CAHEAD && t < nk; ++t) stage(t, !(tail && t == nk - 1));
  ready(0);
  load(F0, 0);
  int64_t t = 0;
  // the unconditional form of steps t and t + 1 needs stage t + 1 + AHEAD whole (not the tail)
  const int64_t nfull = nk - (tail ? 1 : 0);
  for (; t + CAHEAD + 1 < nfull; t += 2) {
    step_full(t, F0, F1);
    step_full(t + 1, F1, F0);
  }
  for (; t < nk; t += 2) {
    step(t, F0, F1);
    if (t + 1 < nk) step(t + 1, F1, F0);
  }

  // epilogue: accumulator (bm, bn) element g <-> tile row pl(bm, g), tile column ql(bn): a lane
  // owns one column of 4 rows, 16 lanes store one 128-byte run
  auto pl = [&](int bm, int g) -> int { return wm * 64 + 16 * bm + kk + 4 * g; };
  auto ql = [&](int bn) -> int { return wn * 64 + 16 * bn + r; };
  double ynv[4];
#pragma unroll
  for (int bn = 0; bn < 4; ++bn) {
    const int64_t j = y0 + ql(bn);
    ynv[bn] = yn[j < n ? j : n - 1];
  }
  const bool full = x0 + CT <= m && y0 + CT <= n;  // workgroup-uniform
#pragma unroll
  for (int bm = 0; bm < 4; ++bm) {
    double xnv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t i = x0 + pl(bm, g);
      xnv[g] = xn[i < m ? i : m - 1];
    }
#pragma unroll
    for (int bn = 0; bn < 4; ++bn) {
      const int64_t col = y0 + ql(bn);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t row = x0 + pl(bm, g);
        const double o = cf_fin<OP>(fmax(fma(-2.0, acc[bm][bn][g], xnv[g] + ynv[bn]), 0.0), scale);
        if (full || (row < m && col < n)) __builtin_nontemporal_store(o, C + row * ldc + col);
      }
    }
  }
}

template <int OP>
int cf_mm_launch(unsigned tiles, hipStream_t s, const double* X, int64_t m, const double* Y, int64_t n, int64_t f,
                 int64_t ldx, int64_t ldy, const double* xn, const double* yn, double* C, int64_t ldc, double scale) {
  hipLaunchKernelGGL(cdist_f64_mm<OP>, dim3(tiles), dim3(256), 0, s, X, m, Y, n, f, ldx, ldy, xn, yn, C, ldc, scale);
  return ha_launch_status();
}

// ------------------------------------------------------------- (b) difference form on the VALU
constexpr int VT = 128, VK = 16, VS = VT + 2;  // tile, features per chunk, LDS row stride (doubles)

template <int OP, bool SYM>
__global__ __launch_bounds__(256, 2) void cdist_f64_vx(const double* __restrict__ X, int64_t m,
                                                       const double* __restrict__ Y, int64_t n, int64_t f,
                                                       int64_t ldx, int64_t ldy, double* __restrict__ C, int64_t ldc,
                                                       double scale, int64_t per_xcd, int vec) {
  static_assert(2 * 2 * VK * VS * 8 <= 80 * 1024, "two workgroups per CU");
  __shared__ __attribute__((aligned(16))) double sm[2][2][VK * VS];  // [buffer][x / y][feature][row]
  const int tid = threadIdx.x;
  const int64_t tiles_n = (n + VT - 1) / VT;
  const int64_t tiles = SYM ? tiles_n * (tiles_n + 1) / 2 : ((m + VT - 1) / VT) * tiles_n;
  const int64_t t = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  if (t >= tiles) return;
  int64_t row0, col0;
  if (SYM) {
    // t -> (i, j >= i): row i holds tiles_n - i tiles; invert the prefix sums with the quadratic
    // formula, then correct the rounding
    const double T = (double)tiles_n;
    int64_t i = (int64_t)((2.0 * T + 1.0 - sqrt((2.0 * T + 1.0) * (2.0 * T + 1.0) - 8.0 * (double)t)) / 2.0);
    auto first = [&](int64_t r) { return r * tiles_n - r * (r - 1) / 2; };
    if (i < 0) i = 0;
    if (i > tiles_n - 1) i = tiles_n - 1;
    while (i > 0 && first(i) > t) --i;
    while (first(i + 1) <= t) ++i;
    row0 = i * VT;
    col0 = (i + (t - first(i))) * VT;
  } else {
    row0 = (t / tiles_n) * VT;
    col0 = (t % tiles_n) * VT;
  }
  const int tr = tid >> 4, tc = tid & 15;
  // staging role: feature column sc of the chunk, tile rows 2 (sq + 16 u) + {0, 1}, u = 0 .. 3
  const int sc = tid & 15, sq = tid >> 4;
  const double* gx[8];
  const double* gy[8];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t a = row0 + 2 * (sq + 16 * u) + j, b = col0 + 2 * (sq + 16 * u) + j;
      gx[2 * u + j] = X + (a < m ? a : m - 1) * ldx;   // clamped: masked at the store
      gy[2 * u + j] = Y + (b < n ? b : n - 1) * ldy;
    }
  double vx[8], vy[8];
  // every load of the chunk issued back to back; features past f - 1 re-read column f - 1 (never
  // summed: the inner loop stops at f)
  auto gload = [&](int64_t k0) {
    const int64_t k = k0 + sc < f ? k0 + sc : f - 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      vx[e] = gx[e][k];
      vy[e] = gy[e][k];
    }
  };
  auto swrite = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      *reinterpret_cast<doublex2*>(&sm[buf][0][sc * VS + 2 * (sq + 16 * u)]) = (doublex2){vx[2 * u], vx[2 * u + 1]};
      *reinterpret_cast<doublex2*>(&sm[buf][1][sc * VS + 2 * (sq + 16 * u)]) = (doublex2){vy[2 * u], vy[2 * u + 1]};
    }
  };

  double acc[8][8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;

  gload(0);
  swrite(0);
  __syncthreads();
  int buf = 0;
  for (int64_t k0 = 0; k0 < f; k0 += VK, buf ^= 1) {
    const bool more = k0 + VK < f;
    if (more) gload(k0 + VK);  // in flight under this chunk's inner loop
    const int kc = (int)(f - k0 < VK ? f - k0 : VK);
    const double* sx = &sm[buf][0][2 * tr];
    const double* sy = &sm[buf][1][2 * tc];
    for (int k = 0; k < kc; ++k) {
      double xv[8], yv[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const doublex2 a = *reinterpret_cast<const doublex2*>(sx + k * VS + 32 * i);
        const doublex2 b = *reinterpret_cast<const doublex2*>(sy + k * VS + 32 * i);
        xv[2 * i] = a[0];
        xv[2 * i + 1] = a[1];
        yv[2 * i] = b[0];
        yv[2 * i + 1] = b[1];
      }
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const double d = xv[a] - yv[b];
          if (OP == OP_L1) acc[a][b] += __builtin_fabs(d);
          else acc[a][b] = __builtin_fma(d, d, acc[a][b]);
        }
    }
    if (more) {
      swrite(buf ^ 1);  // last read in the previous iteration, before its barrier
      __syncthreads();
    }
  }

  // accumulator (a, b) <-> tile row 2 tr + 32 (a / 2) + a % 2, tile column 2 tc + 32 (b / 2) + b % 2
  if (SYM && row0 != col0) {
    // the mirrored tile (col block, row block): own column b becomes a row that holds this
    // thread's 8 values as 4 pairs at columns row0 + 2 tr + 32 i
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int64_t row = col0 + 2 * tc + 32 * (b >> 1) + (b & 1);
      if (row >= n) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t col = row0 + 2 * tr + 32 * i;
        const double o0 = cf_fin<OP>(acc[2 * i][b], scale), o1 = cf_fin<OP>(acc[2 * i + 1][b], scale);
        double* cp = C + row * ldc + col;
        if (vec && col + 1 < m) {
          cf_store2(cp, o0, o1);
        } else {
          if (col < m) cp[0] = o0;
          if (col + 1 < m) cp[1] = o1;
        }
      }
    }
  }
  const bool full = vec && row0 + VT <= m && col0 + VT <= n;  // workgroup-uniform: no per-element tests
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int64_t row = row0 + 2 * tr + 32 * (a >> 1) + (a & 1);
    if (!full && row >= m) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t col = col0 + 2 * tc + 32 * j;
      const double o0 = cf_fin<OP>(acc[a][2 * j], scale), o1 = cf_fin<OP>(acc[a][2 * j + 1], scale);
      double* cp = C + row * ldc + col;
      if (full || (vec && col + 1 < n)) {
        cf_store2(cp, o0, o1);
      } else {
        if (col < n) cp[0] = o0;
        if (col + 1 < n) cp[1] = o1;
      }
    }
  }
}

template <int OP>
int cf_vx_launch(bool sym, unsigned grid, hipStream_t s, const double* X, int64_t m, const double* Y, int64_t n,
                 int64_t f, int64_t ldx, int64_t ldy, double* C, int64_t ldc, double scale, int64_t per_xcd, int vec) {
  if (sym)
    hipLaunchKernelGGL((cdist_f64_vx<OP, true>), dim3(grid), dim3(256), 0, s, X, m, Y, n, f, ldx, ldy, C, ldc, scale,
                       per_xcd, vec);
  else
    hipLaunchKernelGGL((cdist_f64_vx<OP, false>), dim3(grid), dim3(256), 0, s, X, m, Y, n, f, ldx, ldy, C, ldc, scale,
                       per_xcd, vec);
  return ha_launch_status();
}

}  // namespace

// C[m, n] (row-major, ldc >= n) = distances between the rows of X [m, f] and Y [n, f] (feature
// stride 1, row strides ldx, ldy), all fp64. mode: 0 euclidean, 1 squared euclidean, 2 gaussian
// exp(-scale d2) by the quadratic expansion on the fp64 MFMA (needs 16-byte aligned X, Y, even
// ldx, ldy - else HA_BAD_ARG - and ws, m + n doubles of workspace for the row norms);
// 3 manhattan, 4 / 5 / 6 exact euclidean / squared / gaussian on the VALU (any 8-byte alignment,
// any row stride, ws unused). Bit 8 (modes 3-6): symmetric, Y is X - upper tiles computed once and
// mirrored. HA_UNSUPPORTED: more than 2^31 - 1 tiles.
HA_EXPORT int ha_cdist_f64(const double* X, int64_t m, const double* Y, int64_t n, int64_t f, int64_t ldx,
                           int64_t ldy, double* C, int64_t ldc, int mode, double scale, double* ws, void* stream) {
  if (m < 0 || n < 0) return HA_BAD_ARG;
  if (m == 0 || n == 0) return HA_OK;
  if (!X || !Y || !C || f <= 0 || ldc < n || (m > 1 && ldx < f) || (n > 1 && ldy < f)) return HA_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  const bool sym = (mode & 256) != 0;
  mode &= 255;
  if (mode < 0 || mode > 6) return HA_BAD_ARG;
  if (sym && (mode < 3 || X != Y || m != n || ldx != ldy)) return HA_BAD_ARG;
  if (mode >= 3) {
    // 16-byte stores: pairs of columns starting at an even column of a 16-byte aligned, even-ldc C
    const int vec = (ldc % 2 == 0) && ((reinterpret_cast<uintptr_t>(C) & 15) == 0);
    const int64_t tn = (n + VT - 1) / VT;
    const int64_t tiles = sym ? tn * (tn + 1) / 2 : ((m + VT - 1) / VT) * tn;
    const int64_t per_xcd = (tiles + 7) / 8;
    if (per_xcd * 8 > 0x7fffffffLL) return HA_UNSUPPORTED;
    const unsigned g = (unsigned)(per_xcd * 8);
    switch (mode) {
      case 3: return cf_vx_launch<OP_L1>(sym, g, s, X, m, Y, n, f, ldx, ldy, C, ldc, scale, per_xcd, vec);
      case 4: return cf_vx_launch<OP_EUCLID>(sym, g, s, X, m, Y, n, f, ldx, ldy, C, ldc, scale, per_xcd, vec);
      case 5: return cf_vx_launch<OP_SQ>(sym, g, s, X, m, Y, n, f, ldx, ldy, C, ldc, scale, per_xcd, vec);
      default: return cf_vx_launch<OP_GAUSS>(sym, g, s, X, m, Y, n, f, ldx, ldy, C, ldc, scale, per_xcd, vec);
    }
  }
  if (!ws || ldx % 2 || ldy % 2 || (reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(Y) & 15))
    return HA_BAD_ARG;
  const int64_t tiles = ((m + CT - 1) / CT) * ((n + CT - 1) / CT);
  if (tiles > 0x7fffffffLL) return HA_UNSUPPORTED;
  const bool same = X == Y && m == n && ldx == ldy;  // one set of norms
  const int64_t nrows = same ? m : m + n;
  hipLaunchKernelGGL(f64_row_norms, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, s, X, m, ldx, Y,
                     same ? (int64_t)0 : n, ldy, f, ws);
  if (ha_launch_status() != HA_OK) return HA_LAUNCH;
  const double* yn = same ? ws : ws + m;
  switch (mode) {
    case 0: return cf_mm_launch<OP_EUCLID>((unsigned)tiles, s, X, m, Y, n, f, ldx, ldy, ws, yn, C, ldc, scale);
    case 1: return cf_mm_launch<OP_SQ>((unsigned)tiles, s, X, m, Y, n, f, ldx, ldy, ws, yn, C, ldc, scale);
    default: return cf_mm_launch<OP_GAUSS>((unsigned)tiles, s, X, m, Y, n, f, ldx, ldy, ws, yn, C, ldc, scale);
  }
}
