// hipcc-flags: -fno-slp-vectorize -Xclang -target-feature -Xclang -packed-fp32-ops
// Native fp64 GEMM, C = beta C + alpha op(A) op(B), on v_mfma_f64_16x16x4_f64: the throughput
// kernel behind every device float64 product (ht.matmul / dot / cov, the precise CholeskyQR
// products). gemm64 (linalg64.hip: 64 x 64 tiles, guarded scalar loads, two barriers per 16 k) stays
// for the small latency-bound factor updates and as the fallback for unaligned operands.
//
// Modelled on gemm_mid.hip's gemm_f32m, laid out for 8-byte elements:
//   * 128 x 128 output tile, 4 waves of 64 x 64 = 4 x 4 accumulator blocks of 16 x 16 (64 doubles
//     = 128 registers per lane), two workgroups per CU so one tile's epilogue / prologue overlaps
//     the other's MFMAs;
//   * operands global -> LDS through the 4-slot staging ring (64 KB per workgroup) that f64_ring.h
//     describes: the pipeline, both operand images, the K tail and the read behind an odd K;
//   * fragments of stage t + 1 are read into the second register set between stage t's MFMAs;
//   * f64 fragment map: lane -> row lane & 15, k-slot lane >> 4. A stage is two MFMA k-steps
//     s = 0, 1; k-slot kk of step s holds the stage's k = 2 kk + s, for A and B alike:
//       - k-contiguous operand: a lane reads its row's pair kk with ONE ds_read_b128 and feeds
//         both steps;
//       - row-contiguous operand: the rows of each pair of 16 x 16 blocks are INTERLEAVED - block
//         2 p + j, lane r <-> wave row 32 p + 2 r + j - so one ds_read_b128 at k-row 2 kk + s feeds
//         two blocks (again 256 contiguous bytes per 16 lanes); the epilogue maps rows / columns
//         back;
//   * out-of-range rows / columns are clamped at the load and masked at the store;
//   * 1-D grid in the XCD-aware grouped tile order of gemm_f32m (up to 2^31 - 1 tiles), split-K
//     slices on blockIdx.y into fp64 partials, summed in slice order by fd_sum_slices (bit-identical
//     run to run, no atomics); "upper": tiles wholly below the diagonal return at once and only
//     j >= i is written (Gram products).
// Requirements of this kernel: 16-byte aligned A and B, even lda and ldb. Anything else runs on
// gemm64 inside ha_gemm_f64, so a device fp64 product never leaves the hand-written kernels and
// never copies an operand.
//
// Compile figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//   gemm_f64k<AK, BK>   VGPRs  AGPRs  SGPRs  LDS bytes  scratch  occupancy (waves / SIMD)
//   nn (0, 1)            224      0     66     65536        0       2
//   nt (0, 0)            222      0     70     65536        0       2
//   tn (1, 1)            213      0     66     65536        0       2
//   tt (1, 0)            225      0     70     65536        0       2
// 2 waves per SIMD = the planned two workgroups per CU (2 x 64 KB of the 160 KB LDS); the 128
// accumulator registers fit the 256-register budget without AGPRs. The steady-state loop is 64
// MFMAs (two stages), 8 DMAs, 16 ds_read_b128, two "s_waitcnt vmcnt(8)" + s_barrier. The 16-k
// stage / one workgroup per CU alternative was not built: with an f64 MFMA of 64 cycles a stage is
// 2048 MFMA cycles per wave against 8 LDS reads and 4 DMAs, so the tile's prologue and epilogue,
// which only a second workgroup can hide, are what is left to overlap.
#include "f64_ring.h"

#include <type_traits>

namespace {

constexpr int FT = F64_T;           // tile rows / columns
constexpr int FNBUF = 4;            // ring slots
constexpr int FAHEAD = FNBUF - 1;   // stages in flight

// Fragments of one stage for a wave: a[b][s], b[b][s] = block b's operand for MFMA k-step s.
struct FdFrag {
  double a[4][2], b[4][2];
};

// AK: A k-major ([K][M], m contiguous) - else row-major ([M][K], k contiguous).
// BK_: B k-major ([K][N], n contiguous) - else n-major ([N][K], k contiguous).
// Split-K: slice blockIdx.y covers k in [y kps 8, min((y + 1) kps 8, K)) and writes C + y cslice.
template <bool AK, bool BK_>
__global__ __launch_bounds__(256, 2) void gemm_f64k(const double* __restrict__ A, const double* __restrict__ B,
                                                    double* __restrict__ C, int64_t M, int64_t N, int64_t K,
                                                    int64_t lda, int64_t ldb, int64_t ldc, double alpha, int beta,
                                                    int upper, int64_t kps, int64_t cslice) {
  static_assert(FNBUF * F64_STG <= 80 * 1024, "two workgroups per CU");
  __shared__ __attribute__((aligned(16))) unsigned char smem[FNBUF * F64_STG];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int kk = lane >> 4, r = lane & 15;
  const unsigned tn = (unsigned)((N + FT - 1) / FT), tm = (unsigned)((M + FT - 1) / FT);
  const unsigned bid = ha_xcd_remap(blockIdx.x, tm * tn);
  constexpr unsigned GM = 8;
  const unsigned grp = bid / (GM * tn), gfirst = grp * GM;
  const unsigned gsz = tm - gfirst < GM ? tm - gfirst : GM;
  const int64_t m0 = (int64_t)(gfirst + (bid % (GM * tn)) % gsz) * FT, n0 = (int64_t)((bid % (GM * tn)) / gsz) * FT;
  if (upper && n0 + FT <= m0) return;  // wholly below the diagonal (workgroup-uniform, before any barrier)
  {
    const int64_t k0 = (int64_t)blockIdx.y * kps * F64_K;
    A += AK ? k0 * lda : k0;
    B += BK_ ? k0 * ldb : k0;
    K = K - k0 < kps * F64_K ? K - k0 : kps * F64_K;
    C += (int64_t)blockIdx.y * cslice;
  }
  F64Src<!AK> sa;
  F64Src<!BK_> sb;
  sa.init(A, lda, M, m0, lane);
  sb.init(B, ldb, N, n0, lane);
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

  auto stage = [&](int64_t t, bool full) {
    const unsigned dst = sbase + (unsigned)((t % FNBUF) * F64_STG);
    const int64_t k0 = t * F64_K;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      ha_dma16(full ? sa.src(k0, q) : sa.src_clamped(k0, q, K), dst + q * 1024);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      ha_dma16(full ? sb.src(k0, q) : sb.src_clamped(k0, q, K), dst + F64_OP + q * 1024);
    }
  };
  // this wave's own pieces of the tail stage: the values at k >= K become zero
  auto zero_tail = [&](int64_t t) {
    unsigned char* dst = smem + (t % FNBUF) * F64_STG;
    const int64_t k0 = t * F64_K;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      double* pa = reinterpret_cast<double*>(dst + q * 1024 + lane * 16);
      const int64_t ka = sa.kfirst(k0, q);
      if (ka >= K) pa[0] = 0.0;
      if (ka + (AK ? 0 : 1) >= K) pa[1] = 0.0;
      double* pb = reinterpret_cast<double*>(dst + F64_OP + q * 1024 + lane * 16);
      const int64_t kb = sb.kfirst(k0, q);
      if (kb >= K) pb[0] = 0.0;
      if (kb + (BK_ ? 0 : 1) >= K) pb[1] = 0.0;
    }
  };

  // fragment reads of one operand for this wave's 64 rows starting at tile row w0 (see the header)
  auto opnd = [&](const unsigned char* b, int w0, auto kc_tag, double (*o)[2]) __attribute__((always_inline)) {
    constexpr bool kc = decltype(kc_tag)::value;
    if constexpr (kc) {
#pragma unroll
      for (int bl = 0; bl < 4; ++bl) {
        const doublex2 v = *reinterpret_cast<const doublex2*>(b + kk * (FT * 16) + (w0 + 16 * bl + r) * 16);
        o[bl][0] = v[0];
        o[bl][1] = v[1];
      }
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const doublex2 v = *reinterpret_cast<const doublex2*>(b + (2 * kk + s) * (FT * 8) + (w0 + 32 * p + 2 * r) * 8);
          o[2 * p][s] = v[0];
          o[2 * p + 1][s] = v[1];
        }
    }
  };
  auto load = [&](FdFrag& F, int64_t t) {
    const unsigned char* base = smem + (t % FNBUF) * F64_STG;
    opnd(base, wm * 64, std::integral_constant<bool, !AK>(), F.a);
    opnd(base + F64_OP, wn * 64, std::integral_constant<bool, !BK_>(), F.b);
  };

  // accumulator (block bm, bn) element g <-> tile row / column: the f64 16x16x4 C/D map is
  // column = lane & 15, row = (lane >> 4) + 4 g within the block; block <-> rows as in opnd
  auto crow = [&](int bm, int g) -> int {
    const int rho = kk + 4 * g;
    return wm * 64 + (AK ? 32 * (bm >> 1) + 2 * rho + (bm & 1) : 16 * bm + rho);
  };
  auto ccol = [&](int bn) -> int { return wn * 64 + (BK_ ? 32 * (bn >> 1) + 2 * r + (bn & 1) : 16 * bn + r); };

  doublex4 acc[4][4];
#pragma unroll
  for (int bm = 0; bm < 4; ++bm)
#pragma unroll
    for (int bn = 0; bn < 4; ++bn) acc[bm][bn] = (doublex4)(0.0);

  // the stage's 32 MFMAs in two halves (block rows 0-1 / 2-3) around the barrier
  auto mma_half = [&](const FdFrag& F, int part) {
#pragma unroll
    for (int bm = 2 * part; bm < 2 * part + 2; ++bm)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int bn = 0; bn < 4; ++bn)
          acc[bm][bn] = __builtin_amdgcn_mfma_f64_16x16x4f64(F.a[bm][s], F.b[bn][s], acc[bm][bn], 0, 0, 0);
  };

  const int64_t nk = K > 0 ? (K + F64_K - 1) / F64_K : 0;
  const bool tail = (K % F64_K) != 0;
  // stage t landed (this wave's DMA) and visible to every wave; later stages may be in flight
  auto ready = [&](int64_t t) {
    const int64_t later = nk - 1 - t < FAHEAD - 1 ? nk - 1 - t : FAHEAD - 1;  // stages issued after t
    if (tail && t == nk - 1) {
      ha_vm_wait<0>();
      zero_tail(t);
    }
    if (later >= 2) ha_wait_barrier<2 * F64_DPS>();
    else if (later == 1) ha_wait_barrier<F64_DPS>();
    else ha_wait_barrier<0>();
  };
  // steady state: stage t + AHEAD issued (whole, in range), the first half of the MFMAs around
  // it, the counted wait for stage t + 1 + barrier, then stage t + 1's fragment reads between the
  // second half's MFMAs
  auto step_full = [&](int64_t t, const FdFrag& Fc, FdFrag& Fn) {
    stage(t + FAHEAD, true);
    mma_half(Fc, 0);
    __builtin_amdgcn_sched_barrier(0);
    ha_wait_barrier<(FAHEAD - 1) * F64_DPS>();
    load(Fn, t + 1);
    mma_half(Fc, 1);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto step = [&](int64_t t, const FdFrag& Fc, FdFrag& Fn) {
    if (t + FAHEAD < nk) stage(t + FAHEAD, !(tail && t + FAHEAD == nk - 1));
    mma_half(Fc, 0);
    if (t + 1 < nk) {
      ready(t + 1);
      load(Fn, t + 1);
    }
    mma_half(Fc, 1);
  };

  FdFrag F0, F1;
  for (int64_t t = 0; t < FAHEAD && t < nk; ++t) stage(t, !(tail && t == nk - 1));
  if (nk > 0) {
    ready(0);
    load(F0, 0);
  }
  int64_t t = 0;
  // the unconditional form of steps t and t + 1 needs stage t + 1 + AHEAD whole (not the tail)
  const int64_t nfull = nk - (tail ? 1 : 0);
  for (; t + FAHEAD + 1 < nfull; t += 2) {
    step_full(t, F0, F1);
    step_full(t + 1, F1, F0);
  }
  for (; t < nk; t += 2) {
    step(t, F0, F1);
    if (t + 1 < nk) step(t + 1, F1, F0);
  }

  // epilogue: element (bm, bn, g) -> C[m0 + crow(bm, g)][n0 + ccol(bn)]; one block row's C values
  // (16 loads in flight) before its stores when accumulating. Whole tiles with small ldc: a
  // uniform 64-bit tile base + 32-bit lane offsets and no bounds tests.
  const bool full = m0 + FT <= M && n0 + FT <= N && (!upper || n0 >= m0 + FT - 1);
  if (full && ldc < (1 << 23)) {
    double* Ct = C + m0 * ldc + n0;
    const int l = (int)ldc;
#pragma unroll
    for (int bm = 0; bm < 4; ++bm) {
      double cv[4][4];
      if (beta) {
#pragma unroll
        for (int bn = 0; bn < 4; ++bn)
#pragma unroll
          for (int g = 0; g < 4; ++g) cv[bn][g] = Ct[crow(bm, g) * l + ccol(bn)];
      }
#pragma unroll
      for (int bn = 0; bn < 4; ++bn)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          double v = alpha * acc[bm][bn][g];
          if (beta) v += cv[bn][g];
          Ct[crow(bm, g) * l + ccol(bn)] = v;
        }
    }
    return;
  }
#pragma unroll
  for (int bm = 0; bm < 4; ++bm) {
    double cv[4][4];
    if (beta) {
#pragma unroll
      for (int bn = 0; bn < 4; ++bn) {
        const int64_t gc = n0 + ccol(bn);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int64_t gr = m0 + crow(bm, g);
          cv[bn][g] = (gr < M && gc < N && (!upper || gc >= gr)) ? C[gr * ldc + gc] : 0.0;
        }
      }
    }
#pragma unroll
    for (int bn = 0; bn < 4; ++bn) {
      const int64_t gc = n0 + ccol(bn);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t gr = m0 + crow(bm, g);
        double v = alpha * acc[bm][bn][g];
        if (beta) v += cv[bn][g];
        if (gr < M && gc < N && (!upper || gc >= gr)) C[gr * ldc + gc] = v;
      }
    }
  }
}

// out[i, j] = (out[i, j] if beta) + alpha sum over s = 0 .. S - 1 of P[s cslice + i N + j], in
// slice order; upper: only j >= i (the rest of out untouched, those partials never read).
__global__ __launch_bounds__(256) void fd_sum_slices(const double* __restrict__ P, int64_t S, int64_t M, int64_t N,
                                                     int64_t cslice, double* __restrict__ out, int64_t ldo,
                                                     double alpha, int beta, int upper) {
  const int64_t total = M * N;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / N, j = e % N;
    if (upper && j < i) continue;
    double s = 0.0;
    for (int64_t z = 0; z < S; ++z) s += P[z * cslice + e];
    double v = alpha * s;
    if (beta) v += out[i * ldo + j];
    out[i * ldo + j] = v;
  }
}

template <bool AK, bool BK_>
int f64_launch(const double* A, const double* B, double* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
               int64_t ldc, double alpha, int beta, int upper, int64_t kps, int64_t ns, int64_t cslice, hipStream_t s) {
  const int64_t tiles = ((M + FT - 1) / FT) * ((N + FT - 1) / FT);
  const dim3 g((unsigned)tiles, (unsigned)ns), b(256);
  hipLaunchKernelGGL((gemm_f64k<AK, BK_>), g, b, 0, s, A, B, C, M, N, K, lda, ldb, ldc, alpha, beta, upper, kps, cslice);
  return ha_launch_status();
}

// the slice count a request for `slices` becomes: ceil(nk / ceil(nk / slices)) over nk 8-k stages
int64_t f64_norm_slices(int64_t K, int64_t slices) {
  const int64_t nk = (K + F64_K - 1) / F64_K;
  if (nk <= 0 || slices <= 1) return 1;
  if (slices > 65535) slices = 65535;
  const int64_t kps = (nk + slices - 1) / slices;
  return (nk + kps - 1) / kps;
}

}  // namespace

extern "C" int ha_gemm64(const double* A, const double* B, double* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                         int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor, int upper, int64_t batch, int64_t sA,
                         int64_t sB, int64_t sC, double alpha, double beta, void* stream);

// K slices ha_gemm_f64 uses by default for an (M, N, K) product on ncu compute units (1 = no
// split), by the reasoning of the fp32 kernels' split-K: the 128 x 128 tiles fill less than half
// of the 2 ncu workgroup slots, every slice stays >= 64 stages (512 k) deep so the prologue and
// the partial's store are amortised, and the fp64 partials stay below 512 MB.
HA_EXPORT int64_t ha_gemm_f64_slices(int64_t M, int64_t N, int64_t K, int64_t ncu) {
  if (M <= 0 || N <= 0 || K <= 0 || ncu <= 0) return 1;
  const int64_t tiles = ((M + FT - 1) / FT) * ((N + FT - 1) / FT), slots = 2 * ncu;
  if (2 * tiles > slots || K < 2 * 512) return 1;
  int64_t s = (slots + tiles - 1) / tiles;
  if (s > K / 512) s = K / 512;
  const int64_t cap = ((int64_t)1 << 29) / (8 * M * N);
  if (s > cap) s = cap;
  return f64_norm_slices(K, s);
}

// C[M, N] (row-major, ldc >= N) = alpha A B (+ C if beta), fp64 products and accumulation.
// a_kmajor: A element (m, k) at A[k lda + m] (else A[m lda + k]); b_kmajor: B element (k, n) at
// B[k ldb + n] (else B[n ldb + k]). upper: only C(i, j) with j >= i are written. slices > 1 with a
// partial buffer P of slices M N doubles: split-K, partials summed in slice order.
// 16-byte aligned A, B with even lda, ldb run on gemm_f64k; other operands on gemm64 (slices
// ignored), in row chunks below its grid limit.
HA_EXPORT int ha_gemm_f64(const double* A, const double* B, double* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                          int64_t ldb, int64_t ldc, int a_kmajor, int b_kmajor, double alpha, int beta, int upper,
                          int64_t slices, double* P, void* stream) {
  if (M < 0 || N < 0 || K < 0 || !A || !B || !C || ldc < N || (beta != 0 && beta != 1)) return HA_BAD_ARG;
  if (lda < (a_kmajor ? M : K) || ldb < (b_kmajor ? N : K)) return HA_BAD_ARG;
  if (M == 0 || N == 0) return HA_OK;
  hipStream_t s = (hipStream_t)stream;
  if (K == 0 || lda % 2 || ldb % 2 || ((uintptr_t)A & 15) || ((uintptr_t)B & 15)) {
    const int64_t chunk = (int64_t)65535 * 64;
    if (upper && M > chunk) return HA_UNSUPPORTED;
    for (int64_t r0 = 0; r0 < M; r0 += chunk) {
      const int64_t mc = M - r0 < chunk ? M - r0 : chunk;
      const int rc = ha_gemm64(A + (a_kmajor ? r0 : r0 * lda), B, C + r0 * ldc, mc, N, K, lda, ldb, ldc, a_kmajor,
                               b_kmajor, upper, 1, 0, 0, 0, alpha, (double)beta, stream);
      if (rc != HA_OK) return rc;
    }
    return HA_OK;
  }
  const int64_t tiles = ((M + FT - 1) / FT) * ((N + FT - 1) / FT);
  if (tiles > 0x7fffffffLL) return HA_UNSUPPORTED;
  const int64_t nk = (K + F64_K - 1) / F64_K;
  const int64_t ns = P ? f64_norm_slices(K, slices) : 1;
  const int64_t kps = (nk + ns - 1) / ns;
  double* dst = ns > 1 ? P : C;
  const int64_t ldd = ns > 1 ? N : ldc, cslice = ns > 1 ? M * N : 0;
  const double al = ns > 1 ? 1.0 : alpha;
  const int be = ns > 1 ? 0 : beta;
  int rc;
  if (a_kmajor)
    rc = b_kmajor ? f64_launch<true, true>(A, B, dst, M, N, K, lda, ldb, ldd, al, be, upper, kps, ns, cslice, s)
                  : f64_launch<true, false>(A, B, dst, M, N, K, lda, ldb, ldd, al, be, upper, kps, ns, cslice, s);
  else
    rc = b_kmajor ? f64_launch<false, true>(A, B, dst, M, N, K, lda, ldb, ldd, al, be, upper, kps, ns, cslice, s)
                  : f64_launch<false, false>(A, B, dst, M, N, K, lda, ldb, ldd, al, be, upper, kps, ns, cslice, s);
  if (rc != HA_OK || ns == 1) return rc;
  const int64_t g = (M * N + 255) / 256;
  hipLaunchKernelGGL(fd_sum_slices, dim3((unsigned)(g < 16384 ? g : 16384)), dim3(256), 0, s, P, ns, M, N, cslice, C,
                     ldc, alpha, beta, upper);
  return ha_launch_status();
}
