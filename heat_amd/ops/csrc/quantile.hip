// Order statistics on CDNA4 (gfx950): exact multi-rank MSD radix select on the bit-ordered keys of
// float32 / float64 (radix_key.h), the core of percentile and median. The data never moves: every
// pass histograms one digit of the keys that still match a target's prefix, a tiny pick kernel
// extends each target's prefix by the bin that holds its rank. All counters are integers added by
// atomics, so the result is exact and does not depend on scheduling; a split array sums the tables
// of its ranks between a pass and its pick (one int64 all-reduce per digit).
//
//   qsel_rows_small_k  rows of up to 2048 float32 / 1024 float64: a wave per row keeps the keys in
//                      registers and finds every rank by bisection on the key bits (ballot counts
//                      per bit) - one launch, no tables, no LDS
//   qsel_rows_k        contiguous slices, 11-bit digits, (slice, chunk) grid, 16-byte loads
//   qsel_cols_k        axis 0 of a matrix, 8-bit digits, a lane owns the columns of its 16-byte load
//   qsel_pick_k        scan + pick per (slice, target); qsel_finish_k keys -> values, NaN slices
//
// Tables are int64 (a split array's counts pass 2^32). Pass 0: [slices][NB] digit counts and then
// [slices] NaN counts. Pass p >= 1: [slices][R][NB + 64]: NB digit counts, then for bit b < hs (the
// key bits below the prefix) at NB + b the number of matching keys with that bit set, and at NB + 63
// a "mixed" count - see the all-equal rule below.
//
// Compaction: after pick 0 the host reads the largest per-slice count of keys that match any target
// prefix. If it is at most a quarter of the slice, pass 1 also appends the matching keys to a per-slice
// buffer (rows: one slot allocation per wave; order is irrelevant to a selection) and all later
// digits run over that buffer with the rows kernel. Otherwise every digit pass reads the input.
//
// Targets that sit passes out. A target is finished when the keys under its prefix are all equal -
// a bin count of 1 is the special case of one key. Detected with sums only, so that it survives the
// all-reduce: every wave (rows) or workgroup (cols) knows whether ITS matching keys are all equal
// (first key + a flag / running AND and OR); if so it adds its count to the per-bit counters of the
// bits set in that key, if not it adds 1 to "mixed". All keys are equal iff mixed == 0 and every
// per-bit counter is 0 or the bin count: then each unit agrees with every other on every bit, and the
// key is read off the counters. Workgroups whose slice (column tile) has no unfinished target return
// before loading anything, so the remaining launches of a finished call cost a launch each.
//
// Alternatives: a min/max range pre-pass (kmedians.hip's way to skip leading digits) would add a
// full pass to save at most one and was not measured; 8- against 11-bit digits on the rows layout
// and always-compact (cap = whole slice) were not measured either - 11 bits is what fits one 8 KB
// histogram per target, and the quarter cap is the intended value kept as it is. The cols layout has
// 8-bit digits because its histograms are per (column, target).
// Measured whole calls (profiles/quantile.jsonl): median of 1e9 float32 1.77 ms against 0.69 ms for
// the mean pass; all-equal 1e9 float32 (no compaction, finished after pass 1) 4.4 ms; 1e6 rows of 1000
// float32 through qsel_rows_small_k 4.24 ms against 18.9 ms for torch.quantile on the float32 tensor
// (the parent's expression, timed in the same job). A multi-bit bisection was not tried.
#include "radix_key.h"

namespace {

constexpr int QS_MAXR = 32;        // targets per call
constexpr int QS_GROUP = 8;        // targets per launch
constexpr int QS_EXTRA = 64;       // per-bit counters + mixed behind the bins of a pass >= 1 table row
constexpr int QS_ROWS_DB = 11, QS_COLS_DB = 8;
constexpr int QS_SMALL_BYTES = 8192;  // keys per wave in the one-launch kernel: 128 bytes of registers per lane
constexpr int QS_CHS = 257;        // cols histogram stride (bin 256: NaN count in pass 0)

enum { QS_PASS0 = 0, QS_DATA = 1, QS_KEYS = 2 };

typedef unsigned long long u64;

// unsigned-ordered key
template <typename T>
__device__ __forceinline__ typename Tr<T>::U ukey(T x) {
  typedef typename Tr<T>::U U;
  return (U)key_of<T>(x) ^ ((U)1 << (Tr<T>::BITS - 1));
}
template <typename T>
__device__ __forceinline__ T uvalue(u64 u) {
  typedef typename Tr<T>::U U;
  return value_of<T>((typename Tr<T>::S)((U)u ^ ((U)1 << (Tr<T>::BITS - 1))));
}

// ------------------------------------------------------------------------------------ short rows
// A wave per row, four rows per workgroup, no LDS and no barrier. Lane l holds the keys of elements
// l + 64 j, j < KPL, in registers (slots past the row hold the largest key, which is never below a
// probe). Every rank is found by bisection on the key bits: a probe per bit, KPL compare + ballot +
// popcount steps per probe, all wave-uniform. The first form of this kernel kept the keys in LDS and
// walked them in a loop per probe: each step waited for its LDS read (1e6 rows of 1000 float32:
// 27.5 ms); with the keys in registers the probes are independent VALU / SALU work.
template <typename T, int KPL>
__global__ __launch_bounds__(256) void qsel_rows_small_k(const T* __restrict__ x, int64_t nrows, int len, int64_t ld,
                                                         const long long* __restrict__ ranks, int R,
                                                         T* __restrict__ out) {
  typedef typename Tr<T>::U U;
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nrows) return;  // whole waves
  const T* row = x + r * ld;
  U k[KPL];
  bool nan = false;
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int i = lane + 64 * j;
    k[j] = ~(U)0;
    if (i < len) {
      const T v = __builtin_nontemporal_load(row + i);
      nan = nan || v != v;
      k[j] = ukey<T>(v);
    }
  }
  const bool anynan = __ballot(nan) != 0;
  for (int t = 0; t < R; ++t) {
    const int rank = (int)ranks[t];
    U res = 0;
    for (int bit = Tr<T>::BITS - 1; bit >= 0; --bit) {
      const U cand = res | ((U)1 << bit);
      int below = 0;  // keys < cand, wave-uniform
#pragma unroll
      for (int j = 0; j < KPL; ++j) below += __popcll(__ballot(k[j] < cand));
      if (below <= rank) res = cand;
    }
    if (lane == 0) out[(int64_t)t * nrows + r] = anynan ? (T)__builtin_nan("") : uvalue<T>(res);
  }
}

template <typename T>
int qs_small_launch(const T* x, int64_t nrows, int len, int64_t ld, const long long* ranks, int R, T* out,
                    hipStream_t s) {
  const dim3 grid((unsigned)((nrows + 3) / 4));
  if (len <= 256)
    hipLaunchKernelGGL((qsel_rows_small_k<T, 4>), grid, dim3(256), 0, s, x, nrows, len, ld, ranks, R, out);
  else if (len <= 1024)
    hipLaunchKernelGGL((qsel_rows_small_k<T, 16>), grid, dim3(256), 0, s, x, nrows, len, ld, ranks, R, out);
  else
    hipLaunchKernelGGL((qsel_rows_small_k<T, 32>), grid, dim3(256), 0, s, x, nrows, len, ld, ranks, R, out);
  return ha_launch_status();
}

// --------------------------------------------------------------------------------- rows, any length
// Workgroup (slice s = blockIdx.x, chunk = blockIdx.y) of 256 threads. MODE: QS_PASS0 histograms the
// top digit of every key and counts NaNs; QS_DATA / QS_KEYS histogram the digit at `sh` of the
// values / compacted keys whose bits above `hs` equal a live target's prefix, for the targets
// [t0, t0 + tg) (tg <= 8, an LDS histogram of NB + 1 words each); `append` (pass 1, first group)
// also appends the keys that match ANY of the R targets to the slice's compact buffer.
// Every element goes through take() in wave-uniform control flow (out-of-range lanes carry
// ok = false), so ballots see whole waves: a wave whose matching lanes all hold the same key adds
// their number with one LDS atomic - constant and heavily duplicated data would otherwise serialise
// 64 lanes on one bin.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void qsel_rows_k(const T* __restrict__ src, int64_t len, int64_t ld,
                                                   const long long* __restrict__ lens, int nchunks, int db, int hs,
                                                   int sh, int R, int t0, int tg, int append,
                                                   const u64* __restrict__ prefix, const int* __restrict__ live,
                                                   u64* __restrict__ table, typename Tr<T>::U* __restrict__ comp,
                                                   long long* __restrict__ ccnt, int64_t ccap) {
  typedef typename Tr<T>::U U;
  typedef typename Tr<T>::vec vec;
  constexpr int E = Tr<T>::V;
  extern __shared__ unsigned hist[];  // [tg][NB + 1]
  __shared__ U lpre[QS_MAXR];
  __shared__ int llive[QS_MAXR];
  __shared__ U wfirst[4][QS_GROUP];
  __shared__ unsigned wcnt[4][QS_GROUP], wmix[4][QS_GROUP];
  const int NB = 1 << db, HS = NB + 1;
  const int64_t s = blockIdx.x, nslices = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ntab = MODE == QS_PASS0 ? 1 : tg;
  const unsigned wmask = (1u << (hs - sh)) - 1u;
  U pmin = ~(U)0, pmax = 0;
  if (MODE != QS_PASS0) {
    if (tid < R) {
      lpre[tid] = (U)prefix[s * R + tid];
      llive[tid] = live[s * R + tid];
    }
    if (tid < 4 * QS_GROUP) {
      (&wcnt[0][0])[tid] = 0;
      (&wmix[0][0])[tid] = 0;
    }
    __syncthreads();
    const int a0 = append ? 0 : t0, a1 = append ? R : t0 + tg;
    for (int t = a0; t < a1; ++t)
      if (llive[t]) {
        pmin = lpre[t] < pmin ? lpre[t] : pmin;
        pmax = lpre[t] > pmax ? lpre[t] : pmax;
      }
    if (pmin > pmax) return;  // every target of this launch is finished: the whole workgroup leaves
  }
  for (int e = tid; e < ntab * HS; e += 256) hist[e] = 0;
  __syncthreads();
  if (MODE == QS_KEYS) {
    const int64_t have = lens[s];
    len = have < ccap ? have : ccap;
  }
  const int64_t per = (len + nchunks - 1) / nchunks;
  const int64_t c0 = (int64_t)blockIdx.y * per;
  const int64_t c1 = c0 + per < len ? c0 + per : len;
  unsigned nans = 0;

  auto take = [&](T x, bool ok) {
    const U u = MODE == QS_KEYS ? __builtin_bit_cast(U, x) : ukey<T>(x);
    if (MODE == QS_PASS0) {
      const unsigned d = (unsigned)(u >> sh);
      nans += (ok && x != x) ? 1u : 0u;
      const u64 act = __ballot(ok);
      if (!act) return;
      const int fl = __ffsll((long long)act) - 1;
      const unsigned first = __shfl(d, fl, 64);
      if (__ballot(ok && d == first) == act) {
        if (lane == fl) atomicAdd(&hist[first], (unsigned)__popcll(act));
      } else if (ok) {
        atomicAdd(&hist[d], 1u);
      }
    } else {
      const U hp = u >> hs;
      const bool inr = ok && hp >= pmin && hp <= pmax;
      if (!__ballot(inr)) return;  // the common case after pass 0
      if (append) {
        bool any = false;
        if (inr)
          for (int t = 0; t < R; ++t) any = any || (llive[t] && hp == lpre[t]);
        const u64 m = __ballot(any);
        if (m) {
          const int fl = __ffsll((long long)m) - 1;
          u64 base = 0;
          if (lane == fl) base = atomicAdd(reinterpret_cast<u64*>(ccnt + s), (u64)__popcll(m));
          base = __shfl(base, fl, 64);
          const int64_t slot = (int64_t)base + __popcll(m & (((u64)1 << lane) - 1));
          if (any && slot < ccap) comp[s * ccap + slot] = u;  // the host sized ccap from the all-reduced count
        }
      }
      for (int j = 0; j < tg; ++j) {
        if (!llive[t0 + j]) continue;
        const bool mt = inr && hp == lpre[t0 + j];
        const u64 m = __ballot(mt);
        if (!m) continue;
        const int fl = __ffsll((long long)m) - 1;
        const U first = __shfl(u, fl, 64);
        const bool same = __ballot(mt && u == first) == m;
        const unsigned d = (unsigned)(u >> sh) & wmask;
        if (same) {
          if (lane == fl) atomicAdd(&hist[j * HS + d], (unsigned)__popcll(m));
        } else if (mt) {
          atomicAdd(&hist[j * HS + d], 1u);
        }
        if (lane == fl) {  // this wave's all-equal state of target j
          const unsigned c = wcnt[w][j];
          if (!c) wfirst[w][j] = first;
          else if (wfirst[w][j] != first) wmix[w][j] = 1;
          if (!same) wmix[w][j] = 1;
          wcnt[w][j] = c + (unsigned)__popcll(m);
        }
      }
    }
  };

  if (c0 < c1) {
    const T* seg = src + s * ld + c0;
    const int64_t n = c1 - c0;
    int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(seg) & 15)) & 15) / sizeof(T));
    if (head > n) head = n;
    if (head) take(tid < head ? seg[tid] : (T)0, tid < head);
    const int64_t nv = (n - head) / E;
    const vec* v = reinterpret_cast<const vec*>(seg + head);
    auto fetch = [&](int64_t q0, vec (&a)[4]) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t q = q0 + u * 256 + tid;
        a[u] = q < nv ? __builtin_nontemporal_load(v + q) : (vec)((T)0);
      }
    };
    vec nxt[4];
    fetch(0, nxt);
    for (int64_t q0 = 0; q0 < nv; q0 += 4 * 256) {
      vec cur[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
      if (q0 + 4 * 256 < nv) fetch(q0 + 4 * 256, nxt);  // the next loads fly over this batch's LDS atomics
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (q0 + u * 256 >= nv) break;  // uniform
        const bool ok = q0 + u * 256 + tid < nv;
#pragma unroll
        for (int e = 0; e < E; ++e) take(cur[u][e], ok);
      }
    }
    const int64_t i0 = head + nv * E, rem = n - i0;
    if (rem) take(tid < rem ? seg[i0 + tid] : (T)0, tid < rem);
  }
  if (MODE == QS_PASS0 && nans) atomicAdd(&hist[NB], nans);
  __syncthreads();
  for (int e = tid; e < ntab * NB; e += 256) {
    const int j = e >> db, d = e & (NB - 1);
    const unsigned c = hist[j * HS + d];
    if (c) atomicAdd(table + (MODE == QS_PASS0 ? s * NB : (s * R + t0 + j) * (int64_t)(NB + QS_EXTRA)) + d, (u64)c);
  }
  if (MODE == QS_PASS0) {
    if (tid == 0 && hist[NB]) atomicAdd(table + nslices * NB + s, (u64)hist[NB]);
  } else {
    for (int j = 0; j < tg; ++j) {
      const unsigned c = wcnt[w][j];
      if (!c) continue;
      u64* extra = table + (s * R + t0 + j) * (int64_t)(NB + QS_EXTRA) + NB;
      if (wmix[w][j]) {
        if (lane == 0) atomicAdd(extra + 63, (u64)1);
      } else if (lane < hs && (((u64)wfirst[w][j] >> lane) & 1)) {
        atomicAdd(extra + lane, (u64)c);
      }
    }
  }
}

// ------------------------------------------------------------------------------------- columns
// Axis 0 of X[n, ncols]: grid (column tiles of FT, row chunks). As med_walk_k a lane owns the V
// adjacent columns of its 16-byte load, 256 / (FT / V) rows per step, 4 steps in flight. LDS
// histograms [column][target][257] bound the tile: FT = 32 for pass 0, 16 for up to 2 targets, 8 for
// up to 8. All R prefixes of the tile's columns sit in LDS; a key is first tested against its
// column's [min, max] prefix range. Matching keys are rare after pass 0, so the append takes its slot
// with one atomic per key here (the lanes of a wave own different columns). The running AND / OR /
// count of a lane's matching keys stay in registers and reach LDS once.
template <typename T, int TG, bool PASS0>
__global__ __launch_bounds__(256) void qsel_cols_k(const T* __restrict__ X, int64_t n, int ncols, int64_t ld,
                                                   int vec_ok, int nchunks, int hs, int sh, int R, int t0, int tg,
                                                   int append, const u64* __restrict__ prefix,
                                                   const int* __restrict__ live, u64* __restrict__ table,
                                                   typename Tr<T>::U* __restrict__ comp, long long* __restrict__ ccnt,
                                                   int64_t ccap) {
  typedef typename Tr<T>::U U;
  typedef typename Tr<T>::vec vec;
  constexpr int V = Tr<T>::V, FT = TG == 1 ? 32 : (TG == 2 ? 16 : 8), LPR = FT / V, RPB = 256 / LPR;
  constexpr int NB = 256, HS = QS_CHS;
  extern __shared__ unsigned hist[];  // [FT][TG][257]
  __shared__ U lpre[FT][QS_MAXR];
  __shared__ unsigned lmask[FT];
  __shared__ u64 sand[FT * TG], sor[FT * TG];
  __shared__ unsigned scnt[FT * TG];
  const int tid = threadIdx.x, fl = tid % LPR, rl = tid / LPR;
  const int col0 = blockIdx.x * FT, col = col0 + fl * V;
  const unsigned wmask = (1u << (hs - sh)) - 1u;
  U pmin[V], pmax[V];
  unsigned gm[V], am[V];  // live targets of this launch's group / of all R, per owned column
  if (!PASS0) {
    for (int e = tid; e < FT * R; e += 256) {
      const int cl = e / R, t = e % R;
      lpre[cl][t] = col0 + cl < ncols ? (U)prefix[(int64_t)(col0 + cl) * R + t] : (U)0;
    }
    if (tid < FT) {
      unsigned m = 0;
      if (col0 + tid < ncols)
        for (int t = 0; t < R; ++t) m |= live[(int64_t)(col0 + tid) * R + t] ? 1u << t : 0u;
      lmask[tid] = m;
    }
    __syncthreads();
    bool act = false;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      am[q] = lmask[fl * V + q];
      gm[q] = (am[q] >> t0) & ((1u << tg) - 1u);
      const unsigned use = append ? am[q] : gm[q] << t0;
      pmin[q] = ~(U)0;
      pmax[q] = 0;
      for (int t = 0; t < R; ++t)
        if ((use >> t) & 1) {
          const U p = lpre[fl * V + q][t];
          pmin[q] = p < pmin[q] ? p : pmin[q];
          pmax[q] = p > pmax[q] ? p : pmax[q];
        }
      act = act || use != 0;
    }
    if (!__syncthreads_or(act)) return;  // no unfinished target in this column tile
  }
  for (int e = tid; e < FT * TG * HS; e += 256) hist[e] = 0;
  if (tid < FT * TG) {
    sand[tid] = ~(u64)0;
    sor[tid] = 0;
    scnt[tid] = 0;
  }
  __syncthreads();
  U ra[V][TG], ro[V][TG];
  unsigned rc[V][TG];
#pragma unroll
  for (int q = 0; q < V; ++q)
#pragma unroll
    for (int j = 0; j < TG; ++j) {
      ra[q][j] = ~(U)0;
      ro[q][j] = 0;
      rc[q][j] = 0;
    }
  auto take = [&](const vec x) {
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (col + q >= ncols) continue;
      const int cl = fl * V + q;
      const U u = ukey<T>(x[q]);
      if (PASS0) {
        atomicAdd(&hist[cl * HS + (int)(u >> (Tr<T>::BITS - QS_COLS_DB))], 1u);
        if (x[q] != x[q]) atomicAdd(&hist[cl * HS + NB], 1u);
      } else {
        const U hp = u >> hs;
        if (hp < pmin[q] || hp > pmax[q]) continue;
        if (append) {
          bool any = false;
          for (int t = 0; t < R; ++t) any = any || (((am[q] >> t) & 1) && lpre[cl][t] == hp);
          if (any) {
            const int64_t slot = (int64_t)atomicAdd(reinterpret_cast<u64*>(ccnt + col + q), (u64)1);
            if (slot < ccap) comp[(int64_t)(col + q) * ccap + slot] = u;
          }
        }
#pragma unroll
        for (int j = 0; j < TG; ++j)
          if (((gm[q] >> j) & 1) && lpre[cl][t0 + j] == hp) {
            atomicAdd(&hist[(cl * TG + j) * HS + (int)((unsigned)(u >> sh) & wmask)], 1u);
            ra[q][j] &= u;
            ro[q][j] |= u;
            rc[q][j] += 1;
          }
      }
    }
  };
  const int64_t per = (n + nchunks - 1) / nchunks;
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < n ? r0 + per : n;
  int64_t r = r0 + rl;
  for (; r + 3 * RPB < r1; r += 4 * RPB) {
    vec x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = ld_row<T>(X, r + u * RPB, n, ld, col, ncols, vec_ok);
#pragma unroll
    for (int u = 0; u < 4; ++u) take(x[u]);
  }
  for (; r < r1; r += RPB) take(ld_row<T>(X, r, n, ld, col, ncols, vec_ok));
  if (!PASS0) {
#pragma unroll
    for (int q = 0; q < V; ++q)
#pragma unroll
      for (int j = 0; j < TG; ++j)
        if (rc[q][j]) {
          const int e = (fl * V + q) * TG + j;
          atomicAnd(&sand[e], (u64)ra[q][j]);
          atomicOr(&sor[e], (u64)ro[q][j]);
          atomicAdd(&scnt[e], rc[q][j]);
        }
  }
  __syncthreads();
  for (int e = tid; e < FT * TG * NB; e += 256) {
    const int ct = e >> 8, d = e & 255, cl = ct / TG, j = ct % TG;
    const unsigned c = hist[ct * HS + d];
    if (!c || col0 + cl >= ncols) continue;
    if (PASS0)
      atomicAdd(table + (int64_t)(col0 + cl) * NB + d, (u64)c);
    else if (j < tg)
      atomicAdd(table + ((int64_t)(col0 + cl) * R + t0 + j) * (NB + QS_EXTRA) + d, (u64)c);
  }
  if (PASS0) {
    if (tid < FT && col0 + tid < ncols && hist[tid * HS + NB])
      atomicAdd(table + (int64_t)ncols * NB + col0 + tid, (u64)hist[tid * HS + NB]);
  } else {
    const u64 low = ((u64)1 << hs) - 1;
    for (int e = tid; e < FT * TG * 64; e += 256) {
      const int ct = e >> 6, b = e & 63, cl = ct / TG, j = ct % TG;
      const unsigned c = scnt[ct];
      if (!c) continue;  // counted only for live targets of existing columns
      u64* extra = table + ((int64_t)(col0 + cl) * R + t0 + j) * (NB + QS_EXTRA) + NB;
      if ((sand[ct] ^ sor[ct]) & low) {
        if (b == 0) atomicAdd(extra + 63, (u64)1);
      } else if (b < hs && ((sand[ct] >> b) & 1)) {
        atomicAdd(extra + b, (u64)c);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ pick
// A workgroup per slice, a wave per target in turn, on the (all-reduced) table of pass `pass`.
// Pass >= 1 first applies the all-equal rule (file header): the target's key is complete, it is
// finished. Otherwise the wave scans the bins, takes the one that holds the rank, extends the prefix
// by this pass's digit, reduces the rank to the rank inside the bin and stores the bin's count; after
// the last digit the prefix is the key. Pick 0 also copies the slice's NaN count and raises record[0]
// to the number of keys under any target's prefix (ranks ascend, so equal prefixes are adjacent).
__global__ __launch_bounds__(256) void qsel_pick_k(int bits, int db, int pass, int R, int64_t nslices,
                                                   const long long* __restrict__ ranks,
                                                   const u64* __restrict__ table, u64* __restrict__ prefix,
                                                   long long* __restrict__ rank, long long* __restrict__ cnt,
                                                   int* __restrict__ live, u64* __restrict__ key,
                                                   long long* __restrict__ nan, long long* __restrict__ record) {
  __shared__ u64 sp[QS_MAXR];
  __shared__ long long sc[QS_MAXR];
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int NB = 1 << db, BPL = NB / 64;
  const int hs = bits - db * pass, sh = hs > db ? hs - db : 0, wd = hs - sh;
  for (int t = w; t < R; t += 4) {
    const int64_t e = s * R + t;
    if (lane == 0) {
      sp[t] = 0;
      sc[t] = 0;
    }
    if (pass > 0 && !live[e]) continue;
    const u64 pre = pass ? prefix[e] : 0;
    long long r = pass ? rank[e] : ranks[t];
    const u64* tab = table + (pass ? e * (int64_t)(NB + QS_EXTRA) : s * NB);
    if (pass > 0) {
      const u64 c = (u64)cnt[e];
      const u64 o = lane < hs ? tab[NB + lane] : 0;
      const bool bad = o != 0 && o != c;
      if (tab[NB + 63] == 0 && !__ballot(bad)) {
        const u64 low = __ballot(o != 0);
        if (lane == 0) {
          key[e] = (pre << hs) | low;
          live[e] = 0;
        }
        continue;
      }
    }
    const u64* b = tab + lane * BPL;
    long long loc = 0;
    for (int i = 0; i < BPL; ++i) loc += (long long)b[i];
    long long inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    const long long total = __shfl(inc, 63, 64);
    if (total <= 0) {  // no keys at all (an empty array is served by the caller)
      if (lane == 0) {
        key[e] = 0;
        live[e] = 0;
      }
      continue;
    }
    if (r >= total) r = total - 1;
    long long below = inc - loc;
    if (below <= r && r < inc) {
      int d = 0;
      while (d < BPL - 1 && below + (long long)b[d] <= r) below += (long long)b[d++];
      const u64 np = (pre << wd) | (u64)(lane * BPL + d);
      prefix[e] = np;
      rank[e] = r - below;
      cnt[e] = (long long)b[d];
      live[e] = sh ? 1 : 0;
      if (!sh) key[e] = np;
      sp[t] = np;
      sc[t] = (long long)b[d];
    }
  }
  __syncthreads();
  if (pass == 0 && threadIdx.x == 0) {
    long long matched = 0;
    for (int t = 0; t < R; ++t)
      if (t == 0 || sp[t] != sp[t - 1]) matched += sc[t];
    __hip_atomic_fetch_max(record, matched, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    nan[s] = (long long)table[nslices * NB + s];
  }
}

// out [R, slices]: the value of each key, NaN for every rank of a slice that holds a NaN
template <typename T>
__global__ __launch_bounds__(256) void qsel_finish_k(int64_t nslices, int R, const u64* __restrict__ key,
                                                     const long long* __restrict__ nan, T* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nslices * R) return;
  const int64_t s = e / R;
  const int t = (int)(e % R);
  out[(int64_t)t * nslices + s] = nan[s] > 0 ? (T)__builtin_nan("") : uvalue<T>(key[e]);
}

// digit geometry of pass `pass`: bits below the prefix, shift of the digit; false past the last digit
bool qs_digit(int dtype, int layout, int pass, int* db, int* hs, int* sh) {
  const int bits = dtype ? 64 : 32;
  *db = layout ? QS_COLS_DB : QS_ROWS_DB;
  if (pass < 0 || *db * pass >= bits) return false;
  *hs = bits - *db * pass;
  *sh = *hs > *db ? *hs - *db : 0;
  return true;
}

int64_t qs_table_elems(int layout, int64_t slices, int R, int pass) {
  const int64_t NB = (int64_t)1 << (layout ? QS_COLS_DB : QS_ROWS_DB);
  return pass == 0 ? slices * (NB + 1) : slices * R * (NB + QS_EXTRA);
}

template <typename T, int MODE>
int qs_rows_launch(const void* src, int64_t slices, int64_t len, int64_t ld, const long long* lens, int nchunks,
                   int db, int hs, int sh, int R, int t0, int tg, int append, const u64* prefix, const int* live,
                   u64* table, void* comp, long long* ccnt, int64_t ccap, hipStream_t s) {
  const size_t lds = sizeof(unsigned) * (MODE == QS_PASS0 ? 1 : tg) * ((1 << db) + 1);
  if (lds > 48 * 1024)
    hipFuncSetAttribute((const void*)qsel_rows_k<T, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((qsel_rows_k<T, MODE>), dim3((unsigned)slices, (unsigned)nchunks), dim3(256), lds, s,
                     (const T*)src, len, ld, lens, nchunks, db, hs, sh, R, t0, tg, append, prefix, live, table,
                     (typename Tr<T>::U*)comp, ccnt, ccap);
  return ha_launch_status();
}

template <typename T, int TG, bool PASS0>
int qs_cols_launch(const T* X, int64_t n, int ncols, int64_t ld, int nchunks, int hs, int sh, int R, int t0, int tg,
                   int append, const u64* prefix, const int* live, u64* table, void* comp, long long* ccnt,
                   int64_t ccap, hipStream_t s) {
  constexpr int FT = TG == 1 ? 32 : (TG == 2 ? 16 : 8);
  const size_t lds = sizeof(unsigned) * FT * TG * QS_CHS;
  if (lds > 48 * 1024)
    hipFuncSetAttribute((const void*)qsel_cols_k<T, TG, PASS0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)lds);
  const int vec_ok =
      ((reinterpret_cast<uintptr_t>(X) & 15) == 0 && (ld * (int64_t)sizeof(T)) % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL((qsel_cols_k<T, TG, PASS0>), dim3((unsigned)((ncols + FT - 1) / FT), (unsigned)nchunks),
                     dim3(256), lds, s, X, n, ncols, ld, vec_ok, nchunks, hs, sh, R, t0, tg, append, prefix, live,
                     table, (typename Tr<T>::U*)comp, ccnt, ccap);
  return ha_launch_status();
}

template <typename T>
int qs_cols_dispatch(const T* X, int64_t n, int ncols, int64_t ld, int nchunks, int pass, int hs, int sh, int R,
                     int t0, int tg, int append, const u64* prefix, const int* live, u64* table, void* comp,
                     long long* ccnt, int64_t ccap, hipStream_t s) {
  if (pass == 0)
    return qs_cols_launch<T, 1, true>(X, n, ncols, ld, nchunks, hs, sh, R, 0, 1, 0, prefix, live, table, comp, ccnt,
                                      ccap, s);
  if (tg <= 2)
    return qs_cols_launch<T, 2, false>(X, n, ncols, ld, nchunks, hs, sh, R, t0, tg, append, prefix, live, table,
                                       comp, ccnt, ccap, s);
  return qs_cols_launch<T, 8, false>(X, n, ncols, ld, nchunks, hs, sh, R, t0, tg, append, prefix, live, table, comp,
                                     ccnt, ccap, s);
}

bool qs_group_ok(int pass, int R, int t0, int tg) {
  return R >= 1 && R <= QS_MAXR && (pass == 0 || (t0 >= 0 && tg >= 1 && tg <= QS_GROUP && t0 + tg <= R));
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
// dtype: 0 float32, 1 float64. layout: 0 rows (contiguous slices, 11-bit digits), 1 cols (axis 0 of a
// matrix, 8-bit digits). All state is per (slice, target), target fastest: prefix / key u64, rank /
// cnt int64, live int32; nan int64 per slice; record int64 [1] (zeroed by the caller).
HA_EXPORT int ha_qsel_max_targets() { return QS_MAXR; }
HA_EXPORT int ha_qsel_group() { return QS_GROUP; }

// digit passes of a call
HA_EXPORT int ha_qsel_passes(int dtype, int layout) {
  const int db = layout ? QS_COLS_DB : QS_ROWS_DB, bits = dtype ? 64 : 32;
  return (bits + db - 1) / db;
}

// longest row of the one-launch kernel
HA_EXPORT int ha_qsel_small_len(int dtype) { return QS_SMALL_BYTES / (dtype ? 8 : 4); }

// int64 entries of the table of pass `pass`; -1 for arguments the kernels do not serve or a table
// above cap entries (the caller then works on fewer slices at a time)
HA_EXPORT int64_t ha_qsel_table_elems(int layout, int64_t slices, int R, int pass, int64_t cap) {
  if ((layout != 0 && layout != 1) || slices <= 0 || slices > 0x7fffffffLL || R < 1 || R > QS_MAXR || pass < 0)
    return -1;
  const int64_t e = qs_table_elems(layout, slices, R, pass);
  return e > cap ? -1 : e;
}

// out [R, nrows] (x's type): the order statistics ranks[0..R) of every row x[r * ld + i], i < len
HA_EXPORT int ha_qsel_rows_small(const void* x, int dtype, int64_t nrows, int64_t len, int64_t ld,
                                 const void* ranks, int R, void* out, void* stream) {
  if ((dtype != 0 && dtype != 1) || nrows < 0 || len < 1 || R < 1 || !ranks || !out || (nrows > 1 && ld < len))
    return HA_BAD_ARG;
  if (nrows == 0) return HA_OK;
  if (!x) return HA_BAD_ARG;
  if (len > ha_qsel_small_len(dtype) || R > QS_MAXR || (nrows + 3) / 4 > 0x7fffffffLL) return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  return dtype == 0 ? qs_small_launch((const float*)x, nrows, (int)len, ld, (const long long*)ranks, R, (float*)out, s)
                    : qs_small_launch((const double*)x, nrows, (int)len, ld, (const long long*)ranks, R, (double*)out,
                                      s);
}

// One digit pass over contiguous slices. mode 0: the values src[s * ld + i], i < len; mode 1 (pass >=
// 2): the compacted keys comp[s * ccap + i], i < min(ccnt[s], ccap). Pass 0 counts every key into
// table [slices][2048] + [slices] NaN counts; pass p >= 1 counts the targets [t0, t0 + tg) into their
// rows of table [slices][R][2048 + 64] (layout 1: the 8-bit digits and 256 bins of a call that began on
// columns). append (pass 1, mode 0): also append the keys under any
// target's prefix to comp / ccnt (zeroed by the caller). table_elems: the table's size.
HA_EXPORT int ha_qsel_rows_pass(const void* src, int dtype, int layout, int mode, int64_t slices, int64_t len,
                                int64_t ld, int nchunks, int pass, int R, int t0, int tg, int append, const void* prefix,
                                const void* live, void* table, int64_t table_elems, void* comp, void* ccnt,
                                int64_t ccap, void* stream) {
  int db, hs, sh;
  if ((dtype != 0 && dtype != 1) || (mode != 0 && mode != 1) || (layout != 0 && layout != 1) ||
      !qs_digit(dtype, layout, pass, &db, &hs, &sh) ||
      slices < 0 || len < 0 || nchunks < 1 || !qs_group_ok(pass, R, t0, tg) || !table || (slices > 1 && ld < len) ||
      (pass > 0 && (!prefix || !live)) || ((append || mode == 1) && (!comp || !ccnt || ccap < 1)) ||
      (append && (pass != 1 || mode != 0)) || (mode == 1 && pass < 2))
    return HA_BAD_ARG;
  if (slices == 0 || len == 0) return HA_OK;
  if (!src && mode == 0) return HA_BAD_ARG;
  if (slices > 0x7fffffffLL || nchunks > 65535 || (len + nchunks - 1) / nchunks > ((int64_t)1 << 30) ||
      table_elems < qs_table_elems(layout, slices, R, pass))
    return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const u64* pre = (const u64*)prefix;
  const int* lv = (const int*)live;
  u64* tab = (u64*)table;
  long long* cc = (long long*)ccnt;
#define QS_ROWS(T, MODE, SRC, LD)                                                                                \
  qs_rows_launch<T, MODE>(SRC, slices, len, LD, cc, nchunks, db, hs, sh, R, t0, tg, append, pre, lv, tab, comp, cc, \
                          ccap, s)
  if (pass == 0) return dtype == 0 ? QS_ROWS(float, QS_PASS0, src, ld) : QS_ROWS(double, QS_PASS0, src, ld);
  if (mode == 0) return dtype == 0 ? QS_ROWS(float, QS_DATA, src, ld) : QS_ROWS(double, QS_DATA, src, ld);
  return dtype == 0 ? QS_ROWS(float, QS_KEYS, comp, ccap) : QS_ROWS(double, QS_KEYS, comp, ccap);
#undef QS_ROWS
}

// One digit pass over the columns of X[n, ncols] (row stride ld); tables as ha_qsel_rows_pass with 256
// bins, comp [ncols][ccap], ccnt [ncols].
HA_EXPORT int ha_qsel_cols_pass(const void* X, int dtype, int64_t n, int64_t ncols, int64_t ld, int nchunks, int pass,
                                int R, int t0, int tg, int append, const void* prefix, const void* live, void* table,
                                int64_t table_elems, void* comp, void* ccnt, int64_t ccap, void* stream) {
  int db, hs, sh;
  if ((dtype != 0 && dtype != 1) || !qs_digit(dtype, 1, pass, &db, &hs, &sh) || n < 0 || ncols < 0 || nchunks < 1 ||
      !qs_group_ok(pass, R, t0, tg) || !table || (n > 1 && ld < ncols) || (pass > 0 && (!prefix || !live)) ||
      (append && (pass != 1 || !comp || !ccnt || ccap < 1)))
    return HA_BAD_ARG;
  if (n == 0 || ncols == 0) return HA_OK;
  if (!X) return HA_BAD_ARG;
  if (ncols > 0x7fffffffLL - 64 || nchunks > 65535 || table_elems < qs_table_elems(1, ncols, R, pass))
    return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  return dtype == 0 ? qs_cols_dispatch((const float*)X, n, (int)ncols, ld, nchunks, pass, hs, sh, R, t0, tg, append,
                                       (const u64*)prefix, (const int*)live, (u64*)table, comp, (long long*)ccnt,
                                       ccap, s)
                    : qs_cols_dispatch((const double*)X, n, (int)ncols, ld, nchunks, pass, hs, sh, R, t0, tg, append,
                                       (const u64*)prefix, (const int*)live, (u64*)table, comp, (long long*)ccnt,
                                       ccap, s);
}

// pick after pass `pass` (and the caller's all-reduce of the table); ranks [R] int64 ascending
HA_EXPORT int ha_qsel_pick(int dtype, int layout, int64_t slices, int R, int pass, const void* ranks,
                           const void* table, int64_t table_elems, void* prefix, void* rank, void* cnt, void* live,
                           void* key, void* nan, void* record, void* stream) {
  int db, hs, sh;
  if ((dtype != 0 && dtype != 1) || (layout != 0 && layout != 1) || !qs_digit(dtype, layout, pass, &db, &hs, &sh) ||
      slices < 0 || R < 1 || R > QS_MAXR || !ranks || !table || !prefix || !rank || !cnt || !live || !key || !nan ||
      !record)
    return HA_BAD_ARG;
  if (slices == 0) return HA_OK;
  if (slices > 0x7fffffffLL || table_elems < qs_table_elems(layout, slices, R, pass)) return HA_UNSUPPORTED;
  hipLaunchKernelGGL(qsel_pick_k, dim3((unsigned)slices), dim3(256), 0, (hipStream_t)stream, dtype ? 64 : 32, db,
                     pass, R, slices, (const long long*)ranks, (const u64*)table, (u64*)prefix, (long long*)rank,
                     (long long*)cnt, (int*)live, (u64*)key, (long long*)nan, (long long*)record);
  return ha_launch_status();
}

// out [R, slices] in the data type from the finished keys
HA_EXPORT int ha_qsel_finish(int dtype, int64_t slices, int R, const void* key, const void* nan, void* out,
                             void* stream) {
  if ((dtype != 0 && dtype != 1) || slices < 0 || R < 1 || R > QS_MAXR || !key || !nan || !out) return HA_BAD_ARG;
  if (slices == 0) return HA_OK;
  const int64_t blocks = (slices * R + 255) / 256;
  if (blocks > 0x7fffffffLL) return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 0)
    hipLaunchKernelGGL(qsel_finish_k<float>, dim3((unsigned)blocks), dim3(256), 0, s, slices, R, (const u64*)key,
                       (const long long*)nan, (float*)out);
  else
    hipLaunchKernelGGL(qsel_finish_k<double>, dim3((unsigned)blocks), dim3(256), 0, s, slices, R, (const u64*)key,
                       (const long long*)nan, (double*)out);
  return ha_launch_status();
}
