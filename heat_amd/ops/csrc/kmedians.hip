// K-medians / k-medoids on CDNA4 (gfx950), float32 and float64 from one templated source:
//   * l1_assign_k   fused Manhattan assignment: |x - c| register tiles on the VALU with a running
//                   (distance, index) per point - no n x k matrix;
//   * l1_row_k      d_i = sum_j |x_ij - M[label_i, j]| - no n x f difference tensor;
//   * med_*         exact per-(cluster, feature) medians by MSD radix select on the bit-ordered keys
//                   over the counting-sort row order of kmeans.hip (ha_km_label_order), replacing
//                   ~100 bisection passes with n x f 8-byte temporaries by <= 4 (fp32) / 8 (fp64)
//                   histogram passes plus one min/max and one fix-up pass.
// There is no MFMA form of L1: everything here is VALU + LDS.
#include "radix_key.h"

namespace {

// ------------------------------------------------------------------------------ fused L1 assignment
// A workgroup of 256 threads owns L1_PB = 128 points. Threads form a 16 x 16 grid: thread (tr, tc)
// holds the 8 x TCN register tile of points {4 tr + 0..3, 64 + 4 tr + 0..3} x centroids
// {TCN tc + 0..TCN-1} of the current centroid tile (CT = 16 TCN centroids; TCN = 1 serves k <= 16,
// where a 64-wide tile would spend 4 to 8 times the work on padding). Points and centroids go
// through LDS in chunks of L1_FK = 32 features, stored row-major with a row stride of FK + V
// elements: a thread reads V consecutive features of a row with one (fp32) or of two features with
// one (fp64) ds_read_b128, the 16 tc lanes of a point row broadcast, and the strides 36 / 68 words
// keep the 16 centroid rows and the 4 point rows of a wave on distinct banks. Per V features that is
// 8 + TCN reads for 8 TCN V subtract + add-with-abs pairs. The next chunk's 16-byte global loads
// are issued into registers before the current chunk is computed.
// acc += |x - c| runs over the features in index order in the data's precision, so the distance is
// the value of the exact cdist manhattan tile and the label is the first-index argmin of that row.
// Padding (features past f, rows past n) is zero in both operands and adds +0; centroids past k are
// never candidates.
constexpr int L1_PB = 128, L1_FK = 32;

template <typename T, int TCN>
__global__ __launch_bounds__(256, 2) void l1_assign_k(const T* __restrict__ X, int64_t n, int f, int64_t ldx,
                                                      int xvec, const T* __restrict__ C, int k, int64_t ldc,
                                                      int cvec, int* __restrict__ labels, T* __restrict__ mind) {
  typedef typename Tr<T>::vec vec;
  constexpr int V = Tr<T>::V, CT = 16 * TCN, LS = L1_FK + V, VPR = L1_FK / V;
  constexpr int NXV = L1_PB * VPR / 256, NCV = (CT * VPR + 255) / 256;
  __shared__ __attribute__((aligned(16))) T sx[L1_PB * LS];
  __shared__ __attribute__((aligned(16))) T sc[CT * LS];
  const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int64_t row0 = (int64_t)blockIdx.x * L1_PB;
  const int nfc = (f + L1_FK - 1) / L1_FK, nct = (k + CT - 1) / CT, steps = nfc * nct;
  vec xr[NXV], cr[NCV];
  auto load = [&](int s) {
    const int ct = s / nfc, k0 = (s % nfc) * L1_FK;
#pragma unroll
    for (int u = 0; u < NXV; ++u) {
      const int v = tid + 256 * u;
      xr[u] = ld_row<T>(X, row0 + v / VPR, n, ldx, k0 + (v % VPR) * V, f, xvec);
    }
#pragma unroll
    for (int u = 0; u < NCV; ++u) {
      const int v = tid + 256 * u;
      // rows past the tile (CT * VPR < 256) clamp to a row past k: zeros, no load
      cr[u] = ld_row<T>(C, v < CT * VPR ? (int64_t)ct * CT + v / VPR : (int64_t)k, k, ldc, k0 + (v % VPR) * V, f, cvec);
    }
  };
  T acc[8][TCN], best[8];
  int bidx[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    best[a] = (T)__builtin_inf();
    bidx[a] = 0x7FFFFFFF;
#pragma unroll
    for (int b = 0; b < TCN; ++b) acc[a][b] = (T)0;
  }
  load(0);
  for (int s = 0; s < steps; ++s) {
    if (s > 0) __syncthreads();  // the previous chunk's reads are done
#pragma unroll
    for (int u = 0; u < NXV; ++u) {
      const int v = tid + 256 * u;
      *reinterpret_cast<vec*>(sx + (v / VPR) * LS + (v % VPR) * V) = xr[u];
    }
#pragma unroll
    for (int u = 0; u < NCV; ++u) {
      const int v = tid + 256 * u;
      if (v < CT * VPR) *reinterpret_cast<vec*>(sc + (v / VPR) * LS + (v % VPR) * V) = cr[u];
    }
    __syncthreads();
    if (s + 1 < steps) load(s + 1);
#pragma unroll(sizeof(T) == 8 ? 1 : 4)  // fp64: more would spill
    for (int kv = 0; kv < VPR; ++kv) {
      vec xv[8], cv[TCN];
#pragma unroll
      for (int a = 0; a < 8; ++a)
        xv[a] = *reinterpret_cast<const vec*>(sx + ((a >> 2) * 64 + 4 * tr + (a & 3)) * LS + kv * V);
#pragma unroll
      for (int b = 0; b < TCN; ++b) cv[b] = *reinterpret_cast<const vec*>(sc + (TCN * tc + b) * LS + kv * V);
#pragma unroll
      for (int q = 0; q < V; ++q)
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < TCN; ++b) acc[a][b] += __builtin_elementwise_abs(xv[a][q] - cv[b][q]);
    }
    if (s % nfc == nfc - 1) {
      const int c0 = (s / nfc) * CT + TCN * tc;
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < TCN; ++b) {
          const T d = acc[a][b];
          const int c = c0 + b;
          if (c < k && (d < best[a] || (d == best[a] && c < bidx[a]))) {
            best[a] = d;
            bidx[a] = c;
          }
          acc[a][b] = (T)0;
        }
    }
  }
  // the 16 tc lanes of a point are adjacent lanes of one wave: lexicographic (distance, index) min
#pragma unroll
  for (int a = 0; a < 8; ++a) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const T od = __shfl_xor(best[a], o, 64);
      const int oi = __shfl_xor(bidx[a], o, 64);
      if (od < best[a] || (od == best[a] && oi < bidx[a])) {
        best[a] = od;
        bidx[a] = oi;
      }
    }
    const int64_t row = row0 + (a >> 2) * 64 + 4 * tr + (a & 3);
    if (tc == 0 && row < n) {
      labels[row] = bidx[a] == 0x7FFFFFFF ? 0 : bidx[a];  // a row of NaN distances
      if (mind) mind[row] = best[a];
    }
  }
}

// d[i] = sum_j |X[i, j] - M[labels[i], j]| (NaN for a label outside [0, k)): 16 lanes per row, a lane
// sums its 16-byte pieces (stride 16 lanes) in index order, the 16 partials are added by a fixed
// butterfly - the same bits on every run.
template <typename T>
__global__ __launch_bounds__(256) void l1_row_k(const T* __restrict__ X, int64_t n, int f, int64_t ldx, int xvec,
                                                const T* __restrict__ M, int k, int64_t ldm, int mvec,
                                                const int* __restrict__ labels, T* __restrict__ d) {
  typedef typename Tr<T>::vec vec;
  constexpr int V = Tr<T>::V;
  const int g = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int lab = row < n ? labels[row] : -1;
  const bool ok = (unsigned)lab < (unsigned)k;
  T s = (T)0;
  if (ok) {
    for (int col = g * V; col < f; col += 16 * V) {
      const vec x = ld_row<T>(X, row, n, ldx, col, f, xvec);
      const vec m = ld_row<T>(M, lab, k, ldm, col, f, mvec);
#pragma unroll
      for (int q = 0; q < V; ++q) s += __builtin_elementwise_abs(x[q] - m[q]);
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (g == 0 && row < n) d[row] = ok ? s : (T)__builtin_nan("");
}

// ----------------------------------------------------------------------------------- exact medians
// Keys: key_of / value_of of radix_key.h. All tables hold signed keys so that the caller's MAX
// reduction orders them; a minimum travels as the maximum of the complement (~s = -1 - s).
constexpr int MED_SEG = 4096;  // sorted positions per workgroup
constexpr int MED_FT = 64;     // features per workgroup tile
constexpr int MED_HS = 257;    // histogram row stride (256 would put a digit of every feature on one bank)
constexpr int MED_RU = 4;      // rows in flight per thread

__device__ __forceinline__ int med_cluster_of(const int* __restrict__ cstart, int k, int64_t p) {
  int lo = 0, hi = k - 1;  // last c with cstart[c] <= p < cstart[c + 1]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cstart[mid + 1] > p) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// One walk serves the three passes over the data. A workgroup takes MED_SEG positions of the
// counting-sort order and a tile of 64 features, and handles the piece of every cluster inside its
// positions in turn (normally one). It gathers 256 / LPR rows at a time with 16-byte loads; within a
// row a lane owns its V features, so two lanes of a row never touch the same feature's state.
//   MED_MINMAX  out[0] = max ~key, out[1] = max key per (cluster, feature)
//   MED_SELECT  the 8-bit digit of (key - kmin) at this pass's shift, of the keys that match the
//               prefix chosen so far, counted into an LDS histogram [feature][256] and added bin by
//               bin (non-zero bins only) to the global [k, f, 256] table with integer atomics -
//               order-free, so the result does not depend on scheduling
//   MED_FIXUP   out[0] = max ~key over keys > v0, out[1] = number of keys <= v0
// MINMAX and FIXUP reduce their two per-thread values over the rows of a wave by shuffles, over the
// 4 waves in LDS, and issue one global atomic per (cluster piece, feature).
enum { MED_MINMAX = 0, MED_SELECT = 1, MED_FIXUP = 2 };

template <typename T, int MODE>
__global__ __launch_bounds__(256) void med_walk_k(const T* __restrict__ X, int f, int64_t ldx, int xvec,
                                                  const int* __restrict__ order, const int* __restrict__ cstart,
                                                  int k, const typename Tr<T>::S* __restrict__ mm,
                                                  const typename Tr<T>::U* __restrict__ prefix,
                                                  const int* __restrict__ npass, int pass,
                                                  unsigned* __restrict__ table, typename Tr<T>::S* __restrict__ out) {
  typedef typename Tr<T>::vec vec;
  typedef typename Tr<T>::S S;
  typedef typename Tr<T>::U U;
  constexpr int V = Tr<T>::V, BITS = Tr<T>::BITS, LPR = MED_FT / V, RPB = 256 / LPR;
  constexpr S SMIN = (S)((U)1 << (BITS - 1));
  extern __shared__ unsigned hist[];       // MED_SELECT: [MED_FT][MED_HS]
  __shared__ S red[2][4][MED_FT];          // the other modes
  const int tid = threadIdx.x, fl = tid % LPR, rl = tid / LPR, wave = tid >> 6;
  const int col0 = blockIdx.y * MED_FT, col = col0 + fl * V;
  const int64_t nvalid = cstart[k], nent = (int64_t)k * f;
  int64_t p0 = (int64_t)blockIdx.x * MED_SEG;
  if (p0 >= nvalid) return;
  const int64_t p1 = p0 + MED_SEG < nvalid ? p0 + MED_SEG : nvalid;
  int c = med_cluster_of(cstart, k, p0);
  while (p0 < p1) {
    while (cstart[c + 1] <= p0) ++c;  // empty clusters
    const int64_t pe = cstart[c + 1] < p1 ? cstart[c + 1] : p1;
    // this thread's V entries of cluster c
    S smin[V], v0[V];
    U pre[V];
    int shift[V];
    bool act = false;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      shift[q] = -1;
      smin[q] = v0[q] = 0;
      pre[q] = 0;
      if (MODE != MED_MINMAX && col + q < f) {
        const int64_t e = (int64_t)c * f + col + q;
        smin[q] = ~mm[e];
        pre[q] = prefix[e];
        v0[q] = (S)((U)smin[q] + pre[q]);
        if (MODE == MED_SELECT && pass < npass[e]) shift[q] = 8 * (npass[e] - 1 - pass);
        act = act || shift[q] >= 0;
      }
    }
    // entries whose range is exhausted sit the pass out; a piece without active entries loads nothing
    const bool work = MODE != MED_SELECT || __syncthreads_or(act);
    S ra[V], rb[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      ra[q] = SMIN;
      rb[q] = MODE == MED_MINMAX ? SMIN : (S)0;
    }
    if (work) {
      if (MODE == MED_SELECT) {
        for (int e = tid; e < MED_FT * MED_HS; e += 256) hist[e] = 0;
        __syncthreads();
      }
      auto take = [&](const vec x) {
#pragma unroll
        for (int q = 0; q < V; ++q) {
          const S s = key_of<T>(x[q]);
          if (MODE == MED_MINMAX) {
            ra[q] = ~s > ra[q] ? ~s : ra[q];
            rb[q] = s > rb[q] ? s : rb[q];
          } else if (MODE == MED_FIXUP) {
            if (s > v0[q]) ra[q] = ~s > ra[q] ? ~s : ra[q]; else rb[q] += 1;
          } else if (shift[q] >= 0) {
            const U rel = (U)s - (U)smin[q];
            const U hi = shift[q] + 8 >= BITS ? (U)0 : rel >> (shift[q] + 8);
            if (hi == pre[q]) atomicAdd(&hist[(fl * V + q) * MED_HS + (int)((rel >> shift[q]) & 255)], 1u);
          }
        }
      };
      int64_t r = p0 + rl;
      for (; r + (MED_RU - 1) * RPB < pe; r += MED_RU * RPB) {
        int idx[MED_RU];
        vec x[MED_RU];
#pragma unroll
        for (int u = 0; u < MED_RU; ++u) idx[u] = order[r + u * RPB];
#pragma unroll
        for (int u = 0; u < MED_RU; ++u) x[u] = ld_row<T>(X, idx[u], (int64_t)1 << 31, ldx, col, f, xvec);
#pragma unroll
        for (int u = 0; u < MED_RU; ++u) take(x[u]);
      }
      for (; r < pe; r += RPB) take(ld_row<T>(X, order[r], (int64_t)1 << 31, ldx, col, f, xvec));
    }
    if (MODE == MED_SELECT) {
      if (work) {
        __syncthreads();
        for (int e = tid; e < MED_FT * 256; e += 256) {
          const int ft = e >> 8;
          const unsigned v = hist[ft * MED_HS + (e & 255)];
          if (v) atomicAdd(&table[(((int64_t)c * f) + col0 + ft) * 256 + (e & 255)], v);  // only features < f count
        }
        __syncthreads();
      }
    } else {
      // rows of a wave: lanes fl + LPR j; FIXUP's rb is a count, everything else a maximum
#pragma unroll
      for (int q = 0; q < V; ++q) {
#pragma unroll
        for (int o = 32; o >= LPR; o >>= 1) {
          const S oa = __shfl_xor(ra[q], o, 64), ob = __shfl_xor(rb[q], o, 64);
          ra[q] = oa > ra[q] ? oa : ra[q];
          rb[q] = MODE == MED_FIXUP ? rb[q] + ob : (ob > rb[q] ? ob : rb[q]);
        }
        if ((tid & 63) < LPR) {
          red[0][wave][fl * V + q] = ra[q];
          red[1][wave][fl * V + q] = rb[q];
        }
      }
      __syncthreads();
      if (tid < MED_FT && col0 + tid < f) {
        S a = red[0][0][tid], b = red[1][0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const S oa = red[0][w][tid], ob = red[1][w][tid];
          a = oa > a ? oa : a;
          b = MODE == MED_FIXUP ? b + ob : (ob > b ? ob : b);
        }
        const int64_t e = (int64_t)c * f + col0 + tid;
        __hip_atomic_fetch_max(out + e, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (MODE == MED_FIXUP)
          __hip_atomic_fetch_add(out + nent + e, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
          __hip_atomic_fetch_max(out + nent + e, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
    }
    p0 = pe;
  }
}

// per entry after pass 0 (and the caller's reduction of its tables): the number of 8-bit digits in
// which the keys of the entry differ, the rank of the lower middle statistic, an empty prefix; the
// largest digit count over all entries goes to *maxpass
template <typename T>
__global__ __launch_bounds__(256) void med_setup_k(const typename Tr<T>::S* __restrict__ mm,
                                                   const long long* __restrict__ counts, int k, int f,
                                                   typename Tr<T>::U* __restrict__ prefix,
                                                   long long* __restrict__ rank, int* __restrict__ npass,
                                                   int* __restrict__ maxpass) {
  typedef typename Tr<T>::U U;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, nent = (int64_t)k * f;
  if (e >= nent) return;
  const long long cnt = counts[e / f];
  int np = 0;
  if (cnt > 0) {
    const U range = (U)mm[nent + e] - (U)~mm[e];
    const int nbits = range ? 64 - __clzll((unsigned long long)range) : 0;
    np = (nbits + 7) / 8;
  }
  npass[e] = np;
  prefix[e] = 0;
  rank[e] = cnt > 0 ? (cnt - 1) / 2 : 0;
  if (np) atomicMax(maxpass, np);
}

// one wave per active (cluster, feature): scan the 256 bins, take the digit that holds the rank,
// extend the prefix, reduce the rank to the rank inside that bin, clear the bins for the next pass
template <typename U>
__global__ __launch_bounds__(256) void med_pick_k(int64_t nent, int pass, unsigned* __restrict__ table,
                                                  U* __restrict__ prefix, long long* __restrict__ rank,
                                                  const int* __restrict__ npass) {
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (e >= nent || pass >= npass[e]) return;  // whole waves
  uint4* bins = reinterpret_cast<uint4*>(table + e * 256) + lane;
  const uint4 b = *bins;
  const unsigned v[4] = {b.x, b.y, b.z, b.w};
  const long long loc = (long long)v[0] + v[1] + v[2] + v[3];
  long long inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  const long long r = rank[e];
  long long below = inc - loc;
  if (below <= r && r < inc) {
    int d = 0;
    while (d < 3 && below + v[d] <= r) below += v[d++];
    prefix[e] = (U)(prefix[e] << 8) | (U)(4 * lane + d);
    rank[e] = r - below;
  }
  *bins = make_uint4(0u, 0u, 0u, 0u);
}

// lower statistic v0 = kmin + prefix; the upper one (rank count / 2) is v0 when more than that many
// keys are <= v0, else the smallest key above v0; their float64 mean rounded to the data type
template <typename T>
__global__ __launch_bounds__(256) void med_finish_k(const typename Tr<T>::S* __restrict__ mm,
                                                    const typename Tr<T>::U* __restrict__ prefix,
                                                    const long long* __restrict__ counts,
                                                    const typename Tr<T>::S* __restrict__ fx, int k, int f,
                                                    T* __restrict__ med) {
  typedef typename Tr<T>::S S;
  typedef typename Tr<T>::U U;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, nent = (int64_t)k * f;
  if (e >= nent) return;
  const long long cnt = counts[e / f];
  if (cnt <= 0) {
    med[e] = (T)0;
    return;
  }
  const S v0 = (S)((U)~mm[e] + prefix[e]);
  const S hi = (long long)fx[nent + e] >= cnt / 2 + 1 ? v0 : (S)~fx[e];
  med[e] = (T)(((double)value_of<T>(v0) + (double)value_of<T>(hi)) / 2);
}

template <typename T>
int rows_vec(const T* p, int64_t ld) {
  return ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld * (int64_t)sizeof(T)) % 16 == 0) ? 1 : 0;
}

template <typename T>
int l1_assign_launch(const T* X, int64_t n, int f, int64_t ldx, const T* C, int k, int64_t ldc, int* labels, T* mind,
                     hipStream_t s) {
  const dim3 grid((unsigned)((n + L1_PB - 1) / L1_PB));
  if (k <= 16)
    hipLaunchKernelGGL((l1_assign_k<T, 1>), grid, dim3(256), 0, s, X, n, f, ldx, rows_vec(X, ldx), C, k, ldc,
                       rows_vec(C, ldc), labels, mind);
  else
    hipLaunchKernelGGL((l1_assign_k<T, 4>), grid, dim3(256), 0, s, X, n, f, ldx, rows_vec(X, ldx), C, k, ldc,
                       rows_vec(C, ldc), labels, mind);
  return ha_launch_status();
}

template <typename T, int MODE>
int med_walk_launch(const T* X, int64_t n, int f, int64_t ldx, const int* order, const int* cstart, int k,
                    const void* mm, const void* prefix, const int* npass, int pass, unsigned* table, void* out,
                    hipStream_t s) {
  typedef typename Tr<T>::S S;
  typedef typename Tr<T>::U U;
  const size_t lds = MODE == MED_SELECT ? sizeof(unsigned) * MED_FT * MED_HS : 0;
  if (lds > 64 * 1024)
    hipFuncSetAttribute((const void*)med_walk_k<T, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const dim3 grid((unsigned)((n + MED_SEG - 1) / MED_SEG), (unsigned)((f + MED_FT - 1) / MED_FT));
  hipLaunchKernelGGL((med_walk_k<T, MODE>), grid, dim3(256), lds, s, X, f, ldx, rows_vec(X, ldx), order, cstart, k,
                     (const S*)mm, (const U*)prefix, npass, pass, table, (S*)out);
  return ha_launch_status();
}

// shapes the median kernels take: n rows as int32 row ids, 64-feature tiles on grid.y
bool med_shape_ok(int64_t n, int k, int f, int64_t ldx) {
  return n > 0 && n < ((int64_t)1 << 31) && k > 0 && f > 0 && f <= 64 * 65535 && (n == 1 || ldx >= f);
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
// dtype: 0 float32, 1 float64, everywhere below.
HA_EXPORT int ha_l1_point_block() { return L1_PB; }

// centroids per tile of the kernel that serves k
HA_EXPORT int ha_l1_centroid_tile(int k) { return k <= 16 ? 16 : 64; }

// labels [n] int32 = first-index argmin_c sum_j |X[i, j] - C[c, j]|, mind [n] (X's type, may be null)
// that minimum. Rows have feature stride 1 and element alignment; 16-byte loads where a matrix's
// rows are 16-byte aligned.
HA_EXPORT int ha_l1_assign(const void* X, int dtype, int64_t n, int f, int64_t ldx, const void* C, int k, int64_t ldc,
                           int* labels, void* mind, void* stream) {
  if (n < 0 || k <= 0 || f <= 0 || (dtype != 0 && dtype != 1) || (n > 1 && ldx < f) || (k > 1 && ldc < f))
    return HA_BAD_ARG;
  if (n == 0) return HA_OK;
  if (!X || !C || !labels) return HA_BAD_ARG;
  if ((n + L1_PB - 1) / L1_PB > 0x7FFFFFFF) return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  return dtype == 0 ? l1_assign_launch((const float*)X, n, f, ldx, (const float*)C, k, ldc, labels, (float*)mind, s)
                    : l1_assign_launch((const double*)X, n, f, ldx, (const double*)C, k, ldc, labels, (double*)mind, s);
}

// d [n] (X's type) = sum_j |X[i, j] - M[labels[i], j]|
HA_EXPORT int ha_l1_to_label(const void* X, int dtype, int64_t n, int f, int64_t ldx, const void* M, int k,
                             int64_t ldm, const int* labels, void* d, void* stream) {
  if (n < 0 || k <= 0 || f <= 0 || (dtype != 0 && dtype != 1) || (n > 1 && ldx < f) || (k > 1 && ldm < f))
    return HA_BAD_ARG;
  if (n == 0) return HA_OK;
  if (!X || !M || !labels || !d) return HA_BAD_ARG;
  if ((n + 15) / 16 > 0x7FFFFFFF) return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + 15) / 16));
  if (dtype == 0)
    hipLaunchKernelGGL(l1_row_k<float>, grid, dim3(256), 0, s, (const float*)X, n, f, ldx,
                       rows_vec((const float*)X, ldx), (const float*)M, k, ldm, rows_vec((const float*)M, ldm), labels,
                       (float*)d);
  else
    hipLaunchKernelGGL(l1_row_k<double>, grid, dim3(256), 0, s, (const double*)X, n, f, ldx,
                       rows_vec((const double*)X, ldx), (const double*)M, k, ldm, rows_vec((const double*)M, ldm),
                       labels, (double*)d);
  return ha_launch_status();
}

HA_EXPORT int ha_med_segment() { return MED_SEG; }

// bytes of the [k, f, 256] u32 digit table, -1 for k, f <= 0 or a table above cap
HA_EXPORT int64_t ha_med_table_bytes(int k, int f, int64_t cap) {
  if (k <= 0 || f <= 0) return -1;
  const int64_t b = (int64_t)k * f * 1024;
  return b > cap ? -1 : b;
}

// pass 0. mm [2, k, f] keys (int32 / int64), preset to the smallest key: mm[0] = max ~key, mm[1] = max key
HA_EXPORT int ha_med_minmax(const void* X, int dtype, int64_t n, int f, int64_t ldx, const int* order,
                            const int* cstart, int k, void* mm, void* stream) {
  if ((dtype != 0 && dtype != 1) || !med_shape_ok(n, k, f, ldx) || !X || !order || !cstart || !mm) return HA_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  return dtype == 0 ? med_walk_launch<float, MED_MINMAX>((const float*)X, n, f, ldx, order, cstart, k, nullptr, nullptr,
                                                         nullptr, 0, nullptr, mm, s)
                    : med_walk_launch<double, MED_MINMAX>((const double*)X, n, f, ldx, order, cstart, k, nullptr,
                                                          nullptr, nullptr, 0, nullptr, mm, s);
}

// counts [k] int64 (all ranks'); writes prefix [k, f] (uint32 / uint64), rank [k, f] int64, npass [k, f]
// int32, and raises *maxpass (preset 0) to the largest npass
HA_EXPORT int ha_med_setup(int dtype, const void* mm, const void* counts, int k, int f, void* prefix, void* rank,
                           int* npass, int* maxpass, void* stream) {
  if ((dtype != 0 && dtype != 1) || k <= 0 || f <= 0 || !mm || !counts || !prefix || !rank || !npass || !maxpass)
    return HA_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(((int64_t)k * f + 255) / 256));
  if (dtype == 0)
    hipLaunchKernelGGL(med_setup_k<float>, grid, dim3(256), 0, s, (const int*)mm, (const long long*)counts, k, f,
                       (unsigned*)prefix, (long long*)rank, npass, maxpass);
  else
    hipLaunchKernelGGL(med_setup_k<double>, grid, dim3(256), 0, s, (const long long*)mm, (const long long*)counts, k,
                       f, (unsigned long long*)prefix, (long long*)rank, npass, maxpass);
  return ha_launch_status();
}

// select pass: digit counts of this rank's rows into table [k, f, 256] u32 (table_bytes: its size)
HA_EXPORT int ha_med_select(const void* X, int dtype, int64_t n, int f, int64_t ldx, const int* order,
                            const int* cstart, int k, const void* mm, const void* prefix, const int* npass, int pass,
                            void* table, int64_t table_bytes, void* stream) {
  if ((dtype != 0 && dtype != 1) || !med_shape_ok(n, k, f, ldx) || !X || !order || !cstart || !mm || !prefix ||
      !npass || !table || pass < 0 || pass >= (dtype == 0 ? 4 : 8))
    return HA_BAD_ARG;
  if (table_bytes < (int64_t)k * f * 1024) return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  return dtype == 0 ? med_walk_launch<float, MED_SELECT>((const float*)X, n, f, ldx, order, cstart, k, mm, prefix, npass,
                                                         pass, (unsigned*)table, nullptr, s)
                    : med_walk_launch<double, MED_SELECT>((const double*)X, n, f, ldx, order, cstart, k, mm, prefix,
                                                          npass, pass, (unsigned*)table, nullptr, s);
}

// pick after a select pass (and the caller's reduction of the table); leaves the table zero
HA_EXPORT int ha_med_pick(int dtype, int k, int f, int pass, void* table, int64_t table_bytes, void* prefix,
                          void* rank, const int* npass, void* stream) {
  if ((dtype != 0 && dtype != 1) || k <= 0 || f <= 0 || pass < 0 || !table || !prefix || !rank || !npass)
    return HA_BAD_ARG;
  if (table_bytes < (int64_t)k * f * 1024) return HA_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nent = (int64_t)k * f;
  const dim3 grid((unsigned)((nent + 3) / 4));
  if (dtype == 0)
    hipLaunchKernelGGL(med_pick_k<unsigned>, grid, dim3(256), 0, s, nent, pass, (unsigned*)table, (unsigned*)prefix,
                       (long long*)rank, npass);
  else
    hipLaunchKernelGGL(med_pick_k<unsigned long long>, grid, dim3(256), 0, s, nent, pass, (unsigned*)table,
                       (unsigned long long*)prefix, (long long*)rank, npass);
  return ha_launch_status();
}

// fix-up pass. fx [2, k, f] keys: fx[0] preset to the smallest key (max ~key over keys > v0),
// fx[1] preset to 0 (number of keys <= v0)
HA_EXPORT int ha_med_fixup(const void* X, int dtype, int64_t n, int f, int64_t ldx, const int* order,
                           const int* cstart, int k, const void* mm, const void* prefix, void* fx, void* stream) {
  if ((dtype != 0 && dtype != 1) || !med_shape_ok(n, k, f, ldx) || !X || !order || !cstart || !mm || !prefix || !fx)
    return HA_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  return dtype == 0 ? med_walk_launch<float, MED_FIXUP>((const float*)X, n, f, ldx, order, cstart, k, mm, prefix, nullptr,
                                                        0, nullptr, fx, s)
                    : med_walk_launch<double, MED_FIXUP>((const double*)X, n, f, ldx, order, cstart, k, mm, prefix,
                                                         nullptr, 0, nullptr, fx, s);
}

// med [k, f] in the data type (0 for a cluster without members)
HA_EXPORT int ha_med_finish(int dtype, int k, int f, const void* mm, const void* prefix, const void* counts,
                            const void* fx, void* med, void* stream) {
  if ((dtype != 0 && dtype != 1) || k <= 0 || f <= 0 || !mm || !prefix || !counts || !fx || !med) return HA_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(((int64_t)k * f + 255) / 256));
  if (dtype == 0)
    hipLaunchKernelGGL(med_finish_k<float>, grid, dim3(256), 0, s, (const int*)mm, (const unsigned*)prefix,
                       (const long long*)counts, (const int*)fx, k, f, (float*)med);
  else
    hipLaunchKernelGGL(med_finish_k<double>, grid, dim3(256), 0, s, (const long long*)mm,
                       (const unsigned long long*)prefix, (const long long*)counts, (const long long*)fx, k, f,
                       (double*)med);
  return ha_launch_status();
}
