// hipcc-flags: -fno-slp-vectorize
// Native float64 k-means assignment (ha_km_assign_f64, behind ops.kmeans_assign_f64): what device
// float64 input of ht.cluster.KMeans (fit / step / predict / k-means++ seeding) runs on. One fused
// kernel: the scores on v_mfma_f64_16x16x4_f64 and a running argmin in registers, so no n x k
// matrix and no float32 copy of the points exist. The deterministic fp64 update lives beside its
// float32 sibling (kmeans.hip: ha_km_update_f64), the fp64 epilogue in kmeans_finalize.hip.
//
// km64_assign: label(i) = argmin_j s(i, j), s(i, j) = |c_j|^2 - 2 x_i.c_j, ties to the lowest j.
//   * one 4-wave workgroup owns 128 points and walks the centroids in tiles of 128; per centroid
//     tile the features of both (k-contiguous) operands come through the 4-slot staging ring that
//     f64_ring.h describes (pipeline, tail, what any f >= 1 means for the loads);
//   * the CENTROIDS feed the MFMA's A side and the points the B side. Under the f64 16x16x4 C/D map
//     (column = lane & 15, row = (lane >> 4) + 4 g) a lane then owns ONE point and 4 centroids per
//     accumulator block, so the per-tile argmin is in-lane. A wave takes 32 points x all 128
//     centroids of the tile: 8 x 2 blocks, 128 accumulator registers (the budget of cdist_f64_mm);
//   * a lane meets its centroids in ascending index order (block, then g), tile after tile, and
//     compares with strict <, so it keeps the lowest index of its own minimum; the running
//     (score, index) pairs stay in registers across the centroid tiles; a point never crosses waves,
//     so the only cross-lane step is ONE lexicographic (score, index) merge over the 4 lane groups
//     (xor 16, 32) after the last tile. Every score is one MFMA chain over the features in index
//     order plus one fma with |c_j|^2: it depends neither on n nor on the tile the point is in;
//   * |c|^2 comes from f64_row_norms (f64_ring.h) into k doubles of workspace, read per tile in
//     the in-lane argmin (L2 hits); |x|^2 is computed by the same pre-pass only when the distance
//     is asked for: mind = max(0, |x|^2 + best);
//   * out-of-range points are clamped at the load and never stored; out-of-range centroids are
//     clamped at the load and scored +inf. Small k (the k = 8 of the reference benchmark) runs the
//     same kernel with masked centroid columns;
//   * the X stages are re-streamed for every centroid tile (from L2 after the first) and a
//     __syncthreads separates two tiles' rings.
//   Not built: keeping the workgroup's X tile resident in LDS where 128 x f doubles fit beside the
//   ring (f <= 16 at two workgroups per CU), and a narrow-k variant for k < 128.
//   Requirements (made so by the Python wrapper, never by a copy in here): the ring's, on X and C.
//   64-bit offsets.
//
// Compile figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//   kernel           VGPRs  AGPRs  SGPRs  LDS bytes  scratch  occupancy (waves / SIMD)
//   km64_assign<*>    254      0    106     65536        0       2
//   f64_row_norms      12      0     20         0        0       8
//   (kmeans.hip)  ku_gather_det_f64<true / false>  90 / 76 VGPRs, no LDS, no scratch, 5 / 6 waves;
//   ku_reduce_det_f64 36 VGPRs, 8 waves; (kmeans_finalize.hip) km_finalize<double, double> 20 VGPRs.
// 2 waves per SIMD = two workgroups per CU. The stage's fragment reads are split (point blocks and
// centroid blocks 0-3 between the MFMA halves, blocks 4-7 behind the second half) and the in-lane
// argmin is branch-free and ordered block by block: read whole / with a branch per centroid, the
// same kernel needed 328 - 336 bytes of scratch per lane.
//
// Measured (MI355X, tools/microbench/kmeans_f64.py, profiles/kmeans_f64_r09.jsonl; n = 4e6 device
// float64 points, ms of round 0 of 3, rounds within 5 %; "before" = what the same public call ran
// before these kernels, alternating in one process; labels agree with "before" on >= 99.9998 %):
//                   ops.kmeans_assign           ops.kmeans_update          KMeans.step (tol=None)
//     f      k     native    before            native    before           native    before
//    18      8      0.79      0.74 (a)          0.45     12450             1.15     13005
//    18    128      0.82      0.75 (a)          0.29      3037             1.13      3094
//    18   1024      5.73      2.62 (a)          0.27       201             6.08       183
//    64      8      1.36      1.37 (a)          0.62     20178             1.92     20691
//    64    128      1.44      1.38 (a)          0.46      2097             2.05      2062
//    64   1024     10.66      4.81 (a)          0.43       727            11.38       566
//   128      8      2.24      2.28 (a)          1.03     19301             3.23     18987
//   128    128      2.34      2.75 (a)          0.81      1591             3.45      1594
//   128   1024     17.73      9.51 (a)          0.82      1085            18.99      1079
//   200      8      3.18      3.67 (b)          1.68     11902             4.90     11317
//   200    128      3.38      5.71 (b)          1.50      1889             5.19      2058
//   200   1024 (c)  6.73      9.88 (b)          0.47       119             7.50       128
// (a) float32 copy of the points + the fp32 MFMA kernel: not a float64 result (the labels of points
//     whose offset is large against the cluster spacing are wrong), so not a time of the same result
//     and no shape class is routed back to it. (b) addmm + min over an n x k float64 matrix: slower
//     in every class measured, so f > 128 is not routed back either. (c) n = 1e6, so that (b)'s
//     matrix stays at 8 GB. "before" of the update is index_add_ (float64 atomics: seconds per call
//     with few clusters, timed by one call where it takes more than 0.5 s) + bincount.
// At k <= 128 the assignment streams the points once (0.7 TB/s at f = 18, 2.0 TB/s at f = 200); at
// k = 1024 it is matrix-core work: 2 n k f = 1.05 TFLOP in 17.7 ms at f = 128 = 59 TF of fp64 MFMA,
// and 26 TF at f = 18, where each 128-centroid tile pays its own ring prologue and drain for three
// stages. Overlapping a tile's prologue with the previous tile's argmin was not tried.
#include "f64_ring.h"

#include <cmath>

namespace {

// ------------------------------------------------------------------------------ fused assignment
constexpr int KT = F64_T;          // points per workgroup / centroids per tile
constexpr int KNBUF = 4;           // ring slots
constexpr int KAHEAD = KNBUF - 1;  // stages in flight

// Fragments of one stage for a wave: c[b][s] = centroid block b (A side), x[b][s] = point block b
// (B side) for MFMA k-step s.
struct Km64Frag {
  double c[8][2], x[2][2];
};

template <bool MIND>
__global__ __launch_bounds__(256, 2) void km64_assign(const double* __restrict__ X, int64_t n,
                                                      const double* __restrict__ C, int64_t k, int64_t f,
                                                      int64_t ldx, int64_t ldc, const double* __restrict__ cn,
                                                      const double* __restrict__ xn, int* __restrict__ labels,
                                                      double* __restrict__ mind) {
  static_assert(KNBUF * F64_STG <= 80 * 1024, "two workgroups per CU");
  __shared__ __attribute__((aligned(16))) unsigned char smem[KNBUF * F64_STG];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kk = lane >> 4, r = lane & 15;
  const int64_t x0 = (int64_t)blockIdx.x * KT;

  F64Src<> sc, sx;
  sx.init(X, ldx, n, x0, lane);
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

  // the centroids' image first, the points' behind it
  auto stage = [&](int64_t t, bool full) {
    const unsigned dst = sbase + (unsigned)((t % KNBUF) * F64_STG);
    const int64_t k0 = t * F64_K;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      ha_dma16(full ? sc.src(k0, q) : sc.src_clamped(k0, q, f), dst + q * 1024);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      ha_dma16(full ? sx.src(k0, q) : sx.src_clamped(k0, q, f), dst + F64_OP + q * 1024);
    }
  };
  // this wave's own pieces of the tail stage: the values at k >= f become zero
  auto zero_tail = [&](int64_t t) {
    unsigned char* dst = smem + (t % KNBUF) * F64_STG;
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

  // fragment reads: all 8 centroid blocks, the wave's 2 point blocks; lane's row r within a block
  // in two parts: the point blocks and centroid blocks 0-3 (part 0), centroid blocks 4-7 (part 1)
  auto load = [&](Km64Frag& F, int64_t t, int part) {
    const unsigned char* base = smem + (t % KNBUF) * F64_STG + kk * (KT * 16) + r * 16;
#pragma unroll
    for (int b = 4 * part; b < 4 * part + 4; ++b) {
      const doublex2 v = *reinterpret_cast<const doublex2*>(base + (16 * b) * 16);
      F.c[b][0] = v[0];
      F.c[b][1] = v[1];
    }
    if (part) return;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const doublex2 v = *reinterpret_cast<const doublex2*>(base + F64_OP + (32 * wave + 16 * b) * 16);
      F.x[b][0] = v[0];
      F.x[b][1] = v[1];
    }
  };

  doublex4 acc[8][2];
  // the stage's 32 MFMAs in two halves (centroid blocks 0-3 / 4-7) around the barrier; 8
  // independent accumulators between two uses of one
  auto mma_half = [&](const Km64Frag& F, int part) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int bm = 4 * part; bm < 4 * part + 4; ++bm)
#pragma unroll
        for (int bn = 0; bn < 2; ++bn)
          acc[bm][bn] = __builtin_amdgcn_mfma_f64_16x16x4f64(F.c[bm][s], F.x[bn][s], acc[bm][bn], 0, 0, 0);
  };

  const int64_t nk = (f + F64_K - 1) / F64_K;
  const bool tail = (f % F64_K) != 0;
  // stage t landed (this wave's DMA) and visible to every wave; later stages may be in flight
  auto ready = [&](int64_t t) {
    const int64_t later = nk - 1 - t < KAHEAD - 1 ? nk - 1 - t : KAHEAD - 1;  // stages issued after t
    if (tail && t == nk - 1) {
      ha_vm_wait<0>();
      zero_tail(t);
    }
    if (later >= 2) ha_wait_barrier<2 * F64_DPS>();
    else if (later == 1) ha_wait_barrier<F64_DPS>();
    else ha_wait_barrier<0>();
  };
  // steady state (f >= 40): stage t + AHEAD issued whole, the first half of the MFMAs around it,
  // the counted wait for stage t + 1 + barrier, the first part of stage t + 1's fragment reads
  // between the second half's MFMAs and the second part behind them, once this stage's centroid
  // blocks 4-7 are dead (still before the next barrier, so before the slot can be refilled)
  auto step_full = [&](int64_t t, const Km64Frag& Fc, Km64Frag& Fn) {
    stage(t + KAHEAD, true);
    mma_half(Fc, 0);
    __builtin_amdgcn_sched_barrier(0);
    ha_wait_barrier<(KAHEAD - 1) * F64_DPS>();
    load(Fn, t + 1, 0);
    mma_half(Fc, 1);
    __builtin_amdgcn_sched_barrier(0);
    load(Fn, t + 1, 1);
    __builtin_amdgcn_sched_barrier(0);
  };
  // the guarded step: the whole loop for f < 40, and the last stages otherwise
  auto step = [&](int64_t t, const Km64Frag& Fc, Km64Frag& Fn) {
    if (t + KAHEAD < nk) stage(t + KAHEAD, !(tail && t + KAHEAD == nk - 1));
    mma_half(Fc, 0);
    if (t + 1 < nk) {
      ready(t + 1);
      load(Fn, t + 1, 0);
    }
    mma_half(Fc, 1);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) load(Fn, t + 1, 1);
    __builtin_amdgcn_sched_barrier(0);
  };

  // running minimum of the lane's point in block bn: over the centroids j with j % 4 == kk
  double best[2] = {INFINITY, INFINITY};
  int bidx[2] = {0x7fffffff, 0x7fffffff};

  for (int64_t c0 = 0; c0 < k; c0 += KT) {
    sc.init(C, ldc, k, c0, lane);
#pragma unroll
    for (int bm = 0; bm < 8; ++bm)
#pragma unroll
      for (int bn = 0; bn < 2; ++bn) acc[bm][bn] = (doublex4)(0.0);

    Km64Frag F0, F1;
    for (int64_t t = 0; t < KAHEAD && t < nk; ++t) stage(t, !(tail && t == nk - 1));
    ready(0);
    load(F0, 0, 0);
    load(F0, 0, 1);
    int64_t t = 0;
    // the unconditional form of steps t and t + 1 needs stage t + 1 + AHEAD whole (not the tail)
    const int64_t nfull = nk - (tail ? 1 : 0);
    for (; t + KAHEAD + 1 < nfull; t += 2) {
      step_full(t, F0, F1);
      step_full(t + 1, F1, F0);
    }
    for (; t < nk; t += 2) {
      step(t, F0, F1);
      if (t + 1 < nk) step(t + 1, F1, F0);
    }

    // in-lane argmin: accumulator (bm, bn) element g <-> centroid c0 + 16 bm + kk + 4 g (ascending
    // in (bm, g)), point 32 wave + 16 bn + r
#pragma unroll
    for (int bm = 0; bm < 8; ++bm) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t j = c0 + 16 * bm + kk + 4 * g;
        const double cj = cn[j < k ? j : k - 1];
        const double nrm = j < k ? cj : INFINITY;
#pragma unroll
        for (int bn = 0; bn < 2; ++bn) {
          const double s = fma(-2.0, acc[bm][bn][g], nrm);
          const bool lt = s < best[bn];
          best[bn] = lt ? s : best[bn];
          bidx[bn] = lt ? (int)j : bidx[bn];
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // block by block: 4 norms in flight, not 32
    }
    // a fast wave's next prologue must not land in a slot a slow wave still reads
    if (c0 + KT < k) __syncthreads();
  }

  // merge over the 4 lane groups that hold the point: lower score, then lower index
#pragma unroll
  for (int bn = 0; bn < 2; ++bn) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const double os = __shfl_xor(best[bn], o, 64);
      const int oi = __shfl_xor(bidx[bn], o, 64);
      if (os < best[bn] || (os == best[bn] && oi < bidx[bn])) {
        best[bn] = os;
        bidx[bn] = oi;
      }
    }
    const int64_t i = x0 + 32 * wave + 16 * bn + r;
    if (kk == 0 && i < n) {
      labels[i] = bidx[bn] == 0x7fffffff ? 0 : bidx[bn];  // no finite score at all
      if (MIND) mind[i] = fmax(xn[i] + best[bn], 0.0);
    }
  }
}

}  // namespace

// labels[i] (int32) = nearest centroid (squared L2, ties to the lowest index) of row i of X [n, f]
// among the rows of C [k, f]; mind[i] (fp64, may be null) = max(0, |x_i|^2 + min score). All fp64,
// feature stride 1, row strides ldx, ldc. ws: k doubles, k + n when mind is given. Needs 16-byte
// aligned X, C with even ldx, ldc (else HA_BAD_ARG). HA_UNSUPPORTED: k >= 2^31 or more than
// 2^31 - 1 point tiles.
HA_EXPORT int ha_km_assign_f64(const double* X, int64_t n, int64_t f, int64_t ldx, const double* C, int64_t k,
                               int64_t ldc, double* ws, int* labels, double* mind, void* stream) {
  if (n < 0 || k <= 0) return HA_BAD_ARG;
  if (n == 0) return HA_OK;
  if (!X || !C || !ws || !labels || f <= 0 || (n > 1 && ldx < f) || (k > 1 && ldc < f)) return HA_BAD_ARG;
  if (ldx % 2 || ldc % 2 || (reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(C) & 15))
    return HA_BAD_ARG;
  const int64_t tiles = (n + KT - 1) / KT;
  if (k > 0x7fffffffLL || tiles > 0x7fffffffLL) return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nrows = k + (mind ? n : 0);
  if ((nrows + 15) / 16 > 0x7fffffffLL) return HA_UNSUPPORTED;
  hipLaunchKernelGGL(f64_row_norms, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, s, C, k, ldc, X,
                     mind ? n : (int64_t)0, ldx, f, ws);
  if (ha_launch_status() != HA_OK) return HA_LAUNCH;
  if (mind)
    hipLaunchKernelGGL(km64_assign<true>, dim3((unsigned)tiles), dim3(256), 0, s, X, n, C, k, f, ldx, ldc, ws, ws + k,
                       labels, mind);
  else
    hipLaunchKernelGGL(km64_assign<false>, dim3((unsigned)tiles), dim3(256), 0, s, X, n, C, k, f, ldx, ldc, ws,
                       (const double*)nullptr, labels, mind);
  return ha_launch_status();
}
