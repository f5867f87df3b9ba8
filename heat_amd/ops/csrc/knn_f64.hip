// hipcc-flags: -fno-slp-vectorize
// Native float64 k-nearest-neighbour search (ha_knn_f64 + ha_knn_rescore_f64, behind
// ops.cdist_f64(..., topk=k)): what device float64 input of ops.knn_topk, ht.spatial.cdist_topk /
// cdist_argmin and ht.classification.KNeighborsClassifier runs on for k <= 16. No nq x nt matrix, no
// distance tile in HBM and no float32 copy of either operand exist.
//
// kn64_topk: for every query row q_i the k rows t_j with the smallest score s(i, j) = |t_j|^2 - 2 q_i.t_j
// in (score, index) order, equal scores to the lowest index, the k-th place included.
//   * the matrix loop is kmeans_f64.hip's km64_assign: one 4-wave workgroup owns 128 queries and walks
//     T in tiles of 128 rows on v_mfma_f64_16x16x4_f64; T on the MFMA's A side and Q on the B side, so
//     a lane owns ONE query per point block (column = lane & 15) and 4 rows of T per accumulator block
//     (row = (lane >> 4) + 4 g); the features of both operands come through the staging pipeline that
//     f64_ring.h describes (images, counted waits, tail), here with a templated slot count (3 is no
//     power of two, so slots are taken by a 32-bit unsigned modulo) and the tail tests behind an opaque
//     copy of the wave number (below); any f >= 1. Every score is one MFMA chain over the features in
//     index order plus one fma with |t_j|^2 (f64_row_norms): it depends neither on nq nor on the tile
//     or the split column, so exactly duplicated rows of T get bit-identical scores and come out in
//     index order;
//   * SELECTION. 2 x k register lists of (double, int) per lane do not fit beside 128 accumulator
//     registers, so the lists live in LDS: per query k sorted (score, index) entries, stored position-
//     major (entry p of query q at [p][q]: the 16 lanes of a lane group touch 16 neighbouring words).
//     A lane keeps only its query's current k-th score (the threshold) in registers. Per accumulator
//     block (8 scores per lane) the tile pass is 8 fmas, 8 compares (s <= threshold) and ONE wave
//     ballot; only a non-empty ballot enters the insertion path. The four lanes that hold one query
//     (lane >> 4 = 0..3) sit in one wave, so the insertion needs no cross-wave synchronisation: it
//     takes the 8 scores one at a time, ballots again, and serves the lane groups that still want to
//     insert one after the other (each behind an lgkmcnt(0)), every lane inserting into its own query's
//     list with the exact lexicographic (score, index) test against the list's k-th entry as it is in
//     LDS then; the register threshold is re-read once at the end (a stale threshold is only too
//     large: it costs a visit, never an entry). Rows of T beyond nt score NaN and never compare true.
//     About k (1 + ln(rows / k)) insertions per query are expected, so far into T the pass costs what
//     km64_assign's in-lane argmin costs;
//   * LDS: lists of 128 x kmax x 12 bytes (12 KB at kmax = 8, 24 KB at kmax = 16). Two workgroups per
//     CU (80 KB each) are kept for every k: k <= 8 runs the 4-slot ring (64 + 12 = 76 KB), k > 8 a
//     3-slot ring (48 + 24 = 72 KB), i.e. 2 stages in flight instead of 3. The other choice, the 4-slot
//     ring at one workgroup per CU, halves the waves that hide the ring's prologue and drain at every
//     T tile, which is what bounds km64_assign at small f;
//   * few queries: grid.y = splits workgroup columns divide T's tiles; column c writes its lists to
//     part[c][query][k]; splits x k <= 64 so that one rescoring group takes them all.
//
// kn64_rescore<G>: a group of G = 16 or 64 lanes per query, lane l owns candidate l of the
// splits x k partial entries (-1 = none). The exact difference-form squared distance as ONE sequential
// fma chain over the features (16-byte loads), a G-lane bitonic sort of (distance bits, index), the k
// smallest written as (float64, int64), (+inf, -1) where T has fewer than k rows. This one launch
// merges the split columns, replaces the expansion scores by exact distances and orders the result.
//
// Requirements (made so by the Python wrapper): the ring's, on Q and T; the rescoring's 16-byte loads
// need the same and never take the 8 bytes behind an odd f. 64-bit offsets.
//
// Compile figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//   kernel             VGPRs  AGPRs  SGPRs  LDS bytes  scratch  occupancy (waves / SIMD)
//   kn64_topk<8>        253      0    102     77824        0       2
//   kn64_topk<16>       256      0     96     73728        0       2
//   f64_row_norms        12      0     20         0        0       8
//   kn64_rescore<*>      28      0   26-30        0        0       8
// 2 waves per SIMD = two workgroups per CU. Three things kept the lists' code out of scratch: the
// block's 8 scores stay in two vector values picked through selects on the bits of the (wave-uniform)
// score number; the output row and the tail stage's two tests are derived behind an opaque copy of the
// lane / wave number, so they are not carried in registers across the tile loop.
//
// Measured (MI355X, tools/microbench/knn_f64.py, profiles/knn_f64_r10.jsonl; device float64, ms of round
// 1 of 2, rounds within 2 %; "fused" = ops.knn_topk + sqrt, norms and rescoring included; "tiles" = what
// the same ht.spatial.cdist_topk block ran before: exact cdist_f64 tiles in HBM + topk / where / topk /
// gather, timed on 4096 queries and scaled to nq, alternating in one process; neighbour sets agree on
// every compared row; "argmin" = ops.kmeans_assign_f64 with distances on the same shape, the same
// matrix loop without lists):
//                          k = 1                      k = 8                k = 16
//    nq = nt      f    fused   tiles  argmin      fused    tiles       fused    tiles
//      4e4       18     3.04     130    3.90       6.26      132       11.30      132
//      4e4       64     5.54     136    7.06       8.54      137       13.20      138
//      4e4      128     9.23     144   11.55      12.07      146       16.39      146
//    2.5e5       18     80.0    5318    95.1       95.2     5354       118.5     5362
//    2.5e5       64    161.1    5616   169.8      176.0     5675       192.7     5677
//    2.5e5      128    277.1    6146   284.3      291.3     6228       307.4     6255
//      1e6       64                               2553    112775  (one call)
//   nq = 256, nt = 1e6 (split columns):  f = 18: k = 1 1.24 / 23.1, k = 16 23.9 / 23.4;
//                                        f = 128: k = 1 3.12 / 37.7, k = 16 48.4 / 38.6.
// At nq = nt = 2.5e5, f = 128 the pass is matrix-core work: 2 nq nt f = 16 TFLOP in 277 - 307 ms = 52 - 58
// TF of fp64 MFMA; the lists cost 5 % at k = 8 and 11 % at k = 16 there, and no more than the in-lane
// argmin at k = 1. At 4e4 rows a query's list still changes often (k (1 + ln(nt / k)) insertions over
// 313 tiles), and k = 16 takes 1.8 - 3.7 times the k = 1 pass. Few queries: splits x k <= 64 leaves 4
// columns at k = 16, 8 workgroups on 256 CUs, and the tiles win (1.02 x at f = 18, 1.26 x at f = 128):
// ht.spatial.cdist_topk sends that class (k > 8, at most two query tiles, >= 2^19 rows) back to them.
// Not built: a second merge level that would lift the 64-candidate cap of the split columns.
#include "f64_ring.h"

#include <cmath>

namespace {

// --------------------------------------------------------------------------------- fused top-k
constexpr int NT = F64_T;         // queries per workgroup / rows of T per tile
constexpr int NOIDX = 0x7fffffff; // index of an empty list entry (sorts behind every row)

// this wave's LDS writes done and visible to its other lanes; nothing cached across it
__device__ __forceinline__ void kn64_wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Fragments of one stage for a wave: t[b][s] = T block b (A side), q[b][s] = query block b (B side)
// for MFMA k-step s.
struct Kn64Frag {
  double t[8][2], q[2][2];
};

// score e = 2 g + bn of a block for a wave-uniform e, as selects on e's bits over two vector values
// (scores kept in an array and picked through e, however the selects are written, are folded into
// a dynamic index and put into scratch)
__device__ __forceinline__ double kn64_sel8(doublex4 v0, doublex4 v1, int e) {
  const doublex4 w = (e & 1) ? v1 : v0;
  const double lo = (e & 2) ? w[1] : w[0], hi = (e & 2) ? w[3] : w[2];
  return (e & 4) ? hi : lo;
}

// KMAX = 8: 4 ring slots; KMAX = 16: 3 ring slots (see the header)
template <int KMAX>
__global__ __launch_bounds__(256, 2) void kn64_topk(const double* __restrict__ Q, int64_t nq,
                                                    const double* __restrict__ T, int64_t nt, int64_t f,
                                                    int64_t ldq, int64_t ldt, const double* __restrict__ tn, int k,
                                                    double* __restrict__ part_s, int* __restrict__ part_i) {
  constexpr int NBUF = KMAX <= 8 ? 4 : 3;  // ring slots
  constexpr int AHEAD = NBUF - 1;          // stages in flight
  static_assert(NBUF * F64_STG + KMAX * NT * 12 <= 80 * 1024, "two workgroups per CU");
  __shared__ __attribute__((aligned(16))) unsigned char smem[NBUF * F64_STG];
  __shared__ double ls[KMAX * NT];  // list scores, [position][query]
  __shared__ int li[KMAX * NT];     // list indices
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kk = lane >> 4, r = lane & 15;
  const int64_t q0 = (int64_t)blockIdx.x * NT;

  // this split column's tiles of T
  const int64_t ntiles = (nt + NT - 1) / NT, per = (ntiles + gridDim.y - 1) / gridDim.y;
  const int64_t tbeg = (int64_t)blockIdx.y * per * NT;
  const int64_t tend = tbeg + per * NT < nt ? tbeg + per * NT : nt;

  F64Src<> st, sq;
  sq.init(Q, ldq, nq, q0, lane);
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  auto slot = [](int64_t t) { return (unsigned)t % (unsigned)NBUF; };

  // T's image first, the queries' behind it
  auto stage = [&](int64_t t, bool full) {
    const unsigned dst = sbase + slot(t) * F64_STG;
    const int64_t k0 = t * F64_K;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      ha_dma16(full ? st.src(k0, q) : st.src_clamped(k0, q, f), dst + q * 1024);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      ha_dma16(full ? sq.src(k0, q) : sq.src_clamped(k0, q, f), dst + F64_OP + q * 1024);
    }
  };
  // this wave's own pieces of the tail stage: the values at k >= f become zero
  auto zero_tail = [&](int64_t t) {
    unsigned char* dst = smem + slot(t) * F64_STG;
    int w = wave;  // opaque: the two tests below are made here, not hoisted and kept across the tile loop
    asm volatile("" : "+s"(w));
    const int64_t ka = t * F64_K + 2 * w;  // both of this wave's pieces hold the pair ka, ka + 1
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = 2 * wave + i;
      double* pa = reinterpret_cast<double*>(dst + q * 1024 + lane * 16);
      double* pb = reinterpret_cast<double*>(dst + F64_OP + q * 1024 + lane * 16);
      if (ka >= f) pa[0] = pb[0] = 0.0;
      if (ka + 1 >= f) pa[1] = pb[1] = 0.0;
    }
  };

  // fragment reads: all 8 T blocks, the wave's 2 query blocks; lane's row r within a block, in two
  // parts: the query blocks and T blocks 0-3 (part 0), T blocks 4-7 (part 1)
  auto load = [&](Kn64Frag& F, int64_t t, int part) {
    const unsigned char* base = smem + slot(t) * F64_STG + kk * (NT * 16) + r * 16;
#pragma unroll
    for (int b = 4 * part; b < 4 * part + 4; ++b) {
      const doublex2 v = *reinterpret_cast<const doublex2*>(base + (16 * b) * 16);
      F.t[b][0] = v[0];
      F.t[b][1] = v[1];
    }
    if (part) return;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const doublex2 v = *reinterpret_cast<const doublex2*>(base + F64_OP + (32 * wave + 16 * b) * 16);
      F.q[b][0] = v[0];
      F.q[b][1] = v[1];
    }
  };

  doublex4 acc[8][2];
  // the stage's 32 MFMAs in two halves (T blocks 0-3 / 4-7) around the barrier; 8 independent
  // accumulators between two uses of one
  auto mma_half = [&](const Kn64Frag& F, int part) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int bm = 4 * part; bm < 4 * part + 4; ++bm)
#pragma unroll
        for (int bn = 0; bn < 2; ++bn)
          acc[bm][bn] = __builtin_amdgcn_mfma_f64_16x16x4f64(F.t[bm][s], F.q[bn][s], acc[bm][bn], 0, 0, 0);
  };

  const int64_t nk = (f + F64_K - 1) / F64_K;
  const bool tail = (f % F64_K) != 0;
  // stage t landed (this wave's DMA) and visible to every wave; later stages may be in flight
  auto ready = [&](int64_t t) {
    const int64_t later = nk - 1 - t < AHEAD - 1 ? nk - 1 - t : AHEAD - 1;  // stages issued after t
    if (tail && t == nk - 1) {
      ha_vm_wait<0>();
      zero_tail(t);
    }
    if (later >= 2) ha_wait_barrier<2 * F64_DPS>();
    else if (later == 1) ha_wait_barrier<F64_DPS>();
    else ha_wait_barrier<0>();
  };
  // steady state: stage t + AHEAD issued whole, the first half of the MFMAs around it, the counted
  // wait for stage t + 1 + barrier, the first part of stage t + 1's fragment reads between the second
  // half's MFMAs and the second part behind them (before the next barrier, so before the slot of
  // stage t + 1 can be refilled)
  auto step_full = [&](int64_t t, const Kn64Frag& Fc, Kn64Frag& Fn) {
    stage(t + AHEAD, true);
    mma_half(Fc, 0);
    __builtin_amdgcn_sched_barrier(0);
    ha_wait_barrier<(AHEAD - 1) * F64_DPS>();
    load(Fn, t + 1, 0);
    mma_half(Fc, 1);
    __builtin_amdgcn_sched_barrier(0);
    load(Fn, t + 1, 1);
    __builtin_amdgcn_sched_barrier(0);
  };
  // the guarded step: the whole loop for small f, and the last stages otherwise
  auto step = [&](int64_t t, const Kn64Frag& Fc, Kn64Frag& Fn) {
    if (t + AHEAD < nk) stage(t + AHEAD, !(tail && t + AHEAD == nk - 1));
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

  // the wave's own 32 lists start empty; its lanes' thresholds at +inf
#pragma unroll
  for (int p = 0; p < KMAX; ++p) {
    if (lane < 32) {
      ls[p * NT + 32 * wave + lane] = INFINITY;
      li[p * NT + 32 * wave + lane] = NOIDX;
    }
  }
  kn64_wave_lds_sync();
  const int ql = 32 * wave + r;  // the lane's query in block 0; block 1 is 16 further
  const double* lthr = ls + (k - 1) * NT + ql;
  double thr[2] = {INFINITY, INFINITY};

  // insert (s, j) into the sorted list of query q if it is lexicographically below its k-th entry
  auto insert = [&](int q, double s, int j) {
    int p = k - 1;
    const double ks = ls[p * NT + q];
    if (!(s < ks || (s == ks && j < li[p * NT + q]))) return;
    for (; p > 0; --p) {
      const double ps = ls[(p - 1) * NT + q];
      const int pi = li[(p - 1) * NT + q];
      if (ps < s || (ps == s && pi < j)) break;
      ls[p * NT + q] = ps;
      li[p * NT + q] = pi;
    }
    ls[p * NT + q] = s;
    li[p * NT + q] = j;
  };

  for (int64_t c0 = tbeg; c0 < tend; c0 += NT) {
    st.init(T, ldt, nt, c0, lane);
#pragma unroll
    for (int bm = 0; bm < 8; ++bm)
#pragma unroll
      for (int bn = 0; bn < 2; ++bn) acc[bm][bn] = (doublex4)(0.0);

    Kn64Frag F0, F1;
    for (int64_t t = 0; t < AHEAD && t < nk; ++t) stage(t, !(tail && t == nk - 1));
    ready(0);
    load(F0, 0, 0);
    load(F0, 0, 1);
    int64_t t = 0;
    // the unconditional form of steps t and t + 1 needs stage t + 1 + AHEAD whole (not the tail)
    const int64_t nfull = nk - (tail ? 1 : 0);
    for (; t + AHEAD + 1 < nfull; t += 2) {
      step_full(t, F0, F1);
      step_full(t + 1, F1, F0);
    }
    for (; t < nk; t += 2) {
      step(t, F0, F1);
      if (t + 1 < nk) step(t + 1, F1, F0);
    }

    // selection: accumulator (bm, bn) element g <-> row c0 + 16 bm + kk + 4 g of T, query
    // 32 wave + 16 bn + r
#pragma unroll
    for (int bm = 0; bm < 8; ++bm) {
      doublex4 sv0, sv1;  // the block's scores of the lane's query in point block 0 / 1
      bool hit = false;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t j = c0 + 16 * bm + kk + 4 * g;
        const double tj = tn[j < nt ? j : nt - 1];
        const double nrm = j < nt ? tj : NAN;
        sv0[g] = fma(-2.0, acc[bm][0][g], nrm);
        sv1[g] = fma(-2.0, acc[bm][1][g], nrm);
        hit |= sv0[g] <= thr[0] || sv1[g] <= thr[1];
      }
      if (__builtin_amdgcn_ballot_w64(hit) != 0) {  // wave-uniform
#pragma unroll 1
        for (int e = 0; e < 8; ++e) {
          const double s = kn64_sel8(sv0, sv1, e);
          const int bn = e & 1;
          const bool want = s <= (bn ? thr[1] : thr[0]);
          uint64_t m = __builtin_amdgcn_ballot_w64(want);
          const int j = (int)(c0 + 16 * bm + kk + 4 * (e >> 1));
          while (m) {  // the lane groups that want to insert, one after the other
            const int grp = __builtin_ctzll(m) >> 4;
            if (want && kk == grp) insert(ql + 16 * bn, s, j);
            kn64_wave_lds_sync();
            m &= ~(0xffffull << (16 * grp));
          }
        }
        thr[0] = lthr[0];
        thr[1] = lthr[16];
      }
      __builtin_amdgcn_sched_barrier(0);  // block by block: 4 norms in flight, not 32
    }
    // a fast wave's next prologue must not land in a slot a slow wave still reads
    if (c0 + NT < tend) __syncthreads();
  }

  // the wave's 32 lists: lane < 32 writes the k entries of query 32 wave + lane
  kn64_wave_lds_sync();
  int ol = lane;  // opaque: everything below is derived here, not kept in registers across the tile loop
  asm volatile("" : "+v"(ol));
  const int64_t qi = q0 + 32 * wave + ol;
  if (ol < 32 && qi < nq) {
    const int64_t o = ((int64_t)blockIdx.y * nq + qi) * k;
    for (int p = 0; p < k; ++p) {
      const int j = li[p * NT + 32 * wave + ol];
      part_s[o + p] = ls[p * NT + 32 * wave + ol];
      part_i[o + p] = j == NOIDX ? -1 : j;
    }
  }
}

// ------------------------------------------------------------------------------ exact rescoring
template <int G>
__global__ __launch_bounds__(256) void kn64_rescore(const double* __restrict__ Q, int64_t ldq,
                                                    const double* __restrict__ T, int64_t ldt, int64_t nt,
                                                    int64_t nq, int64_t f, const int* __restrict__ cand, int splits,
                                                    int kc, int k, double* __restrict__ dist,
                                                    int64_t* __restrict__ out_idx) {
  const int l = threadIdx.x & (G - 1);
  const int64_t q = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (q >= nq) return;  // the whole G-lane group leaves together (q is uniform in the group)
  int64_t i = -1;
  if (l < splits * kc) {
    const int sp = l / kc;
    i = cand[((int64_t)sp * nq + q) * kc + (l - sp * kc)];
  }
  if (i >= nt) i = -1;  // defensive: an out-of-range candidate is "none", never read
  double d = INFINITY;
  if (i >= 0) {
    const double* qr = Q + q * ldq;
    const double* tr = T + i * ldt;
    double acc = 0.0;
    int64_t j = 0;
    for (; j + 2 <= f; j += 2) {
      const doublex2 a = *reinterpret_cast<const doublex2*>(qr + j);
      const doublex2 b = *reinterpret_cast<const doublex2*>(tr + j);
      const double e0 = a[0] - b[0], e1 = a[1] - b[1];
      acc = fma(e0, e0, acc);
      acc = fma(e1, e1, acc);
    }
    if (j < f) {
      const double e = qr[j] - tr[j];
      acc = fma(e, e, acc);
    }
    d = acc;
  }
  // (distance, index) key: d >= 0 (or +inf / NaN), so its bits order like the value; "none" sorts
  // behind every real candidate of equal distance
  uint64_t kd = (uint64_t)__double_as_longlong(d);
  int ki = i >= 0 ? (int)i : NOIDX;
#pragma unroll
  for (int size = 2; size <= G; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const uint64_t od = (uint64_t)__shfl_xor((unsigned long long)kd, stride, 64);
      const int oi = __shfl_xor(ki, stride, 64);
      const bool ascending = (l & size) == 0 || size == G;
      const bool lower = (l & stride) == 0;
      const bool mine_first = kd < od || (kd == od && ki < oi);
      if (mine_first != (lower == ascending)) {
        kd = od;
        ki = oi;
      }
    }
  }
  if (l < k) {
    dist[q * k + l] = ki == NOIDX ? (double)INFINITY : __longlong_as_double((long long)kd);
    out_idx[q * k + l] = ki == NOIDX ? -1 : (int64_t)ki;
  }
}

bool kn64_operands_ok(const double* Q, int64_t ldq, const double* T, int64_t ldt) {
  return ldq % 2 == 0 && ldt % 2 == 0 && (reinterpret_cast<uintptr_t>(Q) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(T) & 15) == 0;
}

}  // namespace

// Partial top-k lists part_s / part_i [splits, nq, k] (fp64 expansion scores |t|^2 - 2 q.t ascending,
// int32 rows of T, (+inf, -1) where a column has fewer than k rows) of every row of Q [nq, f] among
// the rows of T [nt, f]; column c of the splits takes the c-th share of T's 128-row tiles. All fp64,
// feature stride 1, row strides ldq, ldt. ws: nt doubles. Needs 16-byte aligned Q, T with even ldq,
// ldt (else HA_BAD_ARG). HA_UNSUPPORTED: k > 16, splits k > 64, nt or f >= 2^31 - 128, more than
// 2^31 - 1 query tiles.
HA_EXPORT int ha_knn_f64(const double* Q, int64_t nq, int64_t f, int64_t ldq, const double* T, int64_t nt,
                         int64_t ldt, int k, int splits, double* ws, double* part_s, int* part_i, void* stream) {
  if (nq < 0 || nt <= 0 || k < 1 || splits < 1) return HA_BAD_ARG;
  if (k > 16 || splits * k > 64 || splits > 65535) return HA_UNSUPPORTED;
  if (nq == 0) return HA_OK;
  if (!Q || !T || !ws || !part_s || !part_i || f <= 0 || (nq > 1 && ldq < f) || (nt > 1 && ldt < f))
    return HA_BAD_ARG;
  if (!kn64_operands_ok(Q, ldq, T, ldt)) return HA_BAD_ARG;
  const int64_t tiles = (nq + NT - 1) / NT, lim = 0x7fffffffLL - NT;
  if (nt >= lim || f >= lim || tiles > 0x7fffffffLL) return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(f64_row_norms, dim3((unsigned)((nt + 15) / 16)), dim3(256), 0, s, T, nt, ldt,
                     (const double*)nullptr, (int64_t)0, (int64_t)0, f, ws);
  if (ha_launch_status() != HA_OK) return HA_LAUNCH;
  const dim3 grid((unsigned)tiles, (unsigned)splits);
  if (k <= 8)
    hipLaunchKernelGGL(kn64_topk<8>, grid, dim3(256), 0, s, Q, nq, T, nt, f, ldq, ldt, ws, k, part_s, part_i);
  else
    hipLaunchKernelGGL(kn64_topk<16>, grid, dim3(256), 0, s, Q, nq, T, nt, f, ldq, ldt, ws, k, part_s, part_i);
  return ha_launch_status();
}

// dist [nq, k] fp64 / out_idx [nq, k] int64: the k nearest of each query's splits x kc candidate rows
// cand [splits, nq, kc] (int32, -1 = none; the partial lists of ha_knn_f64) by exact fp64
// difference-form squared distance, equal distances by index, (+inf, -1) behind the last candidate.
// Same operand requirements as ha_knn_f64; k <= splits kc <= 64.
HA_EXPORT int ha_knn_rescore_f64(const double* Q, int64_t ldq, const double* T, int64_t ldt, int64_t nt, int64_t nq,
                                 int64_t f, const int* cand, int splits, int kc, int k, double* dist,
                                 int64_t* out_idx, void* stream) {
  if (nq < 0 || nt <= 0 || f <= 0 || splits < 1 || kc < 1 || k < 1) return HA_BAD_ARG;
  if (splits > 64 || kc > 64 || splits * kc > 64) return HA_UNSUPPORTED;
  if (k > splits * kc) return HA_BAD_ARG;
  if (nq == 0) return HA_OK;
  if (!Q || !T || !cand || !dist || !out_idx || (nq > 1 && ldq < f) || (nt > 1 && ldt < f)) return HA_BAD_ARG;
  if (!kn64_operands_ok(Q, ldq, T, ldt)) return HA_BAD_ARG;
  if (nt >= 0x7fffffffLL) return HA_UNSUPPORTED;
  const int g = splits * kc <= 16 ? 16 : 64;
  const int64_t blocks = (nq + 256 / g - 1) / (256 / g);
  if (blocks > 0x7fffffffLL) return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (g == 16)
    hipLaunchKernelGGL(kn64_rescore<16>, dim3((unsigned)blocks), dim3(256), 0, s, Q, ldq, T, ldt, nt, nq, f, cand,
                       splits, kc, k, dist, out_idx);
  else
    hipLaunchKernelGGL(kn64_rescore<64>, dim3((unsigned)blocks), dim3(256), 0, s, Q, ldq, T, ldt, nt, nq, f, cand,
                       splits, kc, k, dist, out_idx);
  return ha_launch_status();
}
