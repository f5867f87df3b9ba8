// Single-pass third and fourth central moments on CDNA4: (n, mean, M2, M3, M4) per output, the
// HBM-bound core of skew and kurtosis (reference heat/core/statistics.py:562 kurtosis, 1456 skew),
// for float and double input.
//
// Every lane that works on one (output, chunk) segment accumulates the SHIFTED power sums
// p_k = sum (x - K)^k, k = 1..4, in fp64 around ONE shift K per segment, so the lanes' sums combine
// by plain fp64 adds (wave shuffles, four LDS slots) and are converted to central form once per
// segment. fp32 sums would not do: converting shifted sums to M3 and M4 cancels leading digits, and
// skew / kurtosis of float64 data are compared at rtol 1e-8. Chunk partials (five doubles) are
// merged with Pebay's formulas by each output's last-arriving block, in a fixed order (two-level
// group tree, write-through partial stores and arrival tickets as in moments.hip), so results are
// bit-reproducible run to run. Loads are 16-byte and non-temporal: the data is streamed once.
//
// The shift: K = x0 + mean(x_i - x0) over the segment's first up to 64 elements (16 rows in the
// column kernel, where every thread re-reads its sample rows: 64 rows of a 512-row chunk would be
// 12% more traffic, and |mean - K| ~ sigma / 4 already leaves M4 without cancellation). Written
// around the first element x0, not as a plain mean, because sum(c, m times) / m != c in fp64 for
// most m: constant input has all differences zero, K = x0 exactly, every d = 0 and
// M2 = M3 = M4 = 0 exactly.
#include "common.h"

namespace {

typedef double doublex2 __attribute__((ext_vector_type(2)));

template <typename T> struct Vec16;
template <> struct Vec16<float> {
  typedef floatx4 type;
  static constexpr int N = 4;
};
template <> struct Vec16<double> {
  typedef doublex2 type;
  static constexpr int N = 2;
};

struct Pow {
  double p1, p2, p3, p4;
};

struct Mom {
  double n, mean, m2, m3, m4;
};

// 6 fp64 VALU operations (+ a conversion for float input) per element
__device__ __forceinline__ void m4_add(Pow& s, double x, double K) {
  const double d = x - K, d2 = d * d;
  s.p1 += d;
  s.p2 += d2;
  s.p3 = fma(d2, d, s.p3);
  s.p4 = fma(d2, d2, s.p4);
}

// Central form of a segment's shifted sums. A rounding-negative M2 or M4 is clamped with `< 0`, which
// lets a NaN through.
__device__ __forceinline__ Mom m4_from_shifted(double n, double K, const Pow& s) {
  Mom m = {n, 0.0, 0.0, 0.0, 0.0};
  if (n > 0) {
    const double dl = s.p1 / n, dl2 = dl * dl;
    m.mean = K + dl;
    m.m2 = s.p2 - n * dl2;
    m.m3 = s.p3 - 3.0 * dl * s.p2 + 2.0 * n * dl2 * dl;
    m.m4 = s.p4 - 4.0 * dl * s.p3 + 6.0 * dl2 * s.p2 - 3.0 * n * dl2 * dl2;
    if (m.m2 < 0) m.m2 = 0.0;
    if (m.m4 < 0) m.m4 = 0.0;
  }
  return m;
}

// Pebay's pairwise update of (n, mean, M2, M3, M4); an empty side passes the other through
__device__ __forceinline__ Mom pebay(const Mom& a, const Mom& b) {
  if (a.n == 0) return b;
  if (b.n == 0) return a;
  Mom r;
  const double n = a.n + b.n, d = b.mean - a.mean, dn = d / n, dn2 = dn * dn, ab = a.n * b.n;
  r.n = n;
  r.mean = a.mean + dn * b.n;
  r.m2 = a.m2 + b.m2 + d * dn * ab;
  r.m3 = a.m3 + b.m3 + d * dn2 * ab * (a.n - b.n) + 3.0 * dn * (a.n * b.m2 - b.n * a.m2);
  r.m4 = a.m4 + b.m4 + d * dn * dn2 * ab * (a.n * a.n - ab + b.n * b.n) +
         6.0 * dn2 * (a.n * a.n * b.m2 + b.n * b.n * a.m2) + 4.0 * dn * (a.n * b.m3 - b.n * a.m3);
  return r;
}

// quintuples in memory: field k at p[k * stride] (stride 1: packed; stride = outputs: planes)
__device__ __forceinline__ Mom m4_load(const double* p, int64_t stride) {
  return Mom{p[0], p[stride], p[2 * stride], p[3 * stride], p[4 * stride]};
}

__device__ __forceinline__ void m4_store(double* p, int64_t stride, const Mom& m) {
  p[0] = m.n;
  p[stride] = m.mean;
  p[2 * stride] = m.m2;
  p[3 * stride] = m.m3;
  p[4 * stride] = m.m4;
}

__device__ __forceinline__ void m4_store_wt(double* p, int64_t stride, const Mom& m) {
  ha_store_wt(p, m.n);
  ha_store_wt(p + stride, m.mean);
  ha_store_wt(p + 2 * stride, m.m2);
  ha_store_wt(p + 3 * stride, m.m3);
  ha_store_wt(p + 4 * stride, m.m4);
}

__device__ __forceinline__ Mom wave_pebay(Mom t) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Mom u;
    u.n = __shfl_xor(t.n, o, 64);
    u.mean = __shfl_xor(t.mean, o, 64);
    u.m2 = __shfl_xor(t.m2, o, 64);
    u.m3 = __shfl_xor(t.m3, o, 64);
    u.m4 = __shfl_xor(t.m4, o, 64);
    t = pebay(t, u);
  }
  return t;
}

// Pebay merge of one quintuple per thread over a 256-thread block (wave butterflies, then the 4
// wave results in wave order); valid in thread 0. sh: 4 x 5 doubles of LDS.
__device__ __forceinline__ Mom m4_block_merge(Mom t, double (*sh)[5]) {
  t = wave_pebay(t);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) m4_store(sh[w], 1, t);
  __syncthreads();
  Mom acc = m4_load(sh[0], 1);
  for (int k = 1; k < 4; ++k) acc = pebay(acc, m4_load(sh[k], 1));
  return acc;
}

// Pebay merge of the quintuples at p + q * step, q in [q0, q1), in q order; 4 loaded per round
__device__ __forceinline__ Mom m4_merge_strided(const double* p, int q0, int q1, int64_t step, int64_t stride) {
  Mom t = {0.0, 0.0, 0.0, 0.0, 0.0};
  int q = q0;
  for (; q + 4 <= q1; q += 4) {
    Mom v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = m4_load(p + (int64_t)(q + u) * step, stride);
#pragma unroll
    for (int u = 0; u < 4; ++u) t = pebay(t, v[u]);
  }
  for (; q < q1; ++q) t = pebay(t, m4_load(p + (int64_t)q * step, stride));
  return t;
}

// Shift of the segment seg[0, n), n >= 1, the same value in every lane of every wave that calls it
template <typename T>
__device__ __forceinline__ double m4_shift(const T* seg, int64_t n, int lane) {
  const int m = n < 64 ? (int)n : 64;
  const double x0 = (double)seg[0];
  const double v = lane < m ? (double)seg[lane] - x0 : 0.0;
  return x0 + ha_wave_sum_d(v) / (double)m;
}

// Thread t of NT adds its share of seg[0, n): a scalar head up to 16-byte alignment (fewer than
// 16 / sizeof(T) elements), the 16-byte body with 4 loads in flight, a scalar tail.
template <typename T, int NT>
__device__ __forceinline__ void m4_accum(const T* seg, int64_t n, int t, double K, Pow& s) {
  typedef typename Vec16<T>::type V;
  constexpr int E = Vec16<T>::N;
  int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(seg) & 15)) & 15) / sizeof(T));
  if (head > n) head = n;
  if (t < head) m4_add(s, (double)seg[t], K);
  const int64_t nv = (n - head) / E;
  const V* v = reinterpret_cast<const V*>(seg + head);
  int64_t q = t;
  for (; q + 3 * NT < nv; q += 4 * NT) {
    V a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = __builtin_nontemporal_load(v + q + u * NT);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < E; ++e) m4_add(s, (double)a[u][e], K);
  }
  {  // at most 3 vectors are left for this thread (q + 3 NT >= nv): all loaded before the first use - a
     // load-use loop here put 3 serial HBM latencies into every short row of the wave-per-row kernel
    V a[3];
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (q + u * NT < nv) a[u] = __builtin_nontemporal_load(v + q + u * NT);
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (q + u * NT < nv) {
#pragma unroll
        for (int e = 0; e < E; ++e) m4_add(s, (double)a[u][e], K);
      }
  }
  for (int64_t i = head + nv * E + t; i < n; i += NT) m4_add(s, (double)seg[i], K);
}

__device__ __forceinline__ Pow wave_pow_sum(Pow s) {
  s.p1 = ha_wave_sum_d(s.p1);
  s.p2 = ha_wave_sum_d(s.p2);
  s.p3 = ha_wave_sum_d(s.p3);
  s.p4 = ha_wave_sum_d(s.p4);
  return s;
}

// rows: x[r * ld + i], i in [0, len). Grid.x = nrows * nchunks, a block per (row, chunk), nchunks > 1.
// part: packed quintuples, chunk partials at (r * nchunks + c) * 5, then group partials at
// (nrows * nchunks + r * ngroups + grp) * 5. out: planes, field k of row r at out[k * nrows + r].
template <typename T>
__global__ __launch_bounds__(256) void m4_rows(const T* __restrict__ x, int64_t nrows, int64_t len, int64_t ld,
                                               int nchunks, int G, double* __restrict__ part,
                                               double* __restrict__ out, unsigned* __restrict__ arrive) {
  const int64_t g = blockIdx.x;
  const int64_t r = g / nchunks;
  const int c = (int)(g % nchunks);
  const int64_t per = (len + nchunks - 1) / nchunks;
  const int64_t c0 = (int64_t)c * per;
  const int64_t c1 = c0 + per < len ? c0 + per : len;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  __shared__ double sh[4][5];
  Pow s = {0.0, 0.0, 0.0, 0.0};
  double K = 0.0;
  if (c0 < c1) {  // the same for the whole block (a late chunk of a short row can be empty)
    const T* seg = x + r * ld + c0;
    K = m4_shift(seg, c1 - c0, lane);
    m4_accum<T, 256>(seg, c1 - c0, tid, K, s);
  }
  s = wave_pow_sum(s);
  if (lane == 0) {
    sh[w][0] = s.p1;
    sh[w][1] = s.p2;
    sh[w][2] = s.p3;
    sh[w][3] = s.p4;
  }
  __syncthreads();
  if (tid == 0) {
    Pow t = {sh[0][0], sh[0][1], sh[0][2], sh[0][3]};
    for (int k = 1; k < 4; ++k) {
      t.p1 += sh[k][0];
      t.p2 += sh[k][1];
      t.p3 += sh[k][2];
      t.p4 += sh[k][3];
    }
    // handed to the row's last block
    m4_store_wt(part + g * 5, 1, m4_from_shifted((double)(c1 > c0 ? c1 - c0 : 0), K, t));
  }
  // two-level tree as in mom_rows: the last-arriving block of each group of G consecutive chunks
  // merges the group (one partial per thread, fixed lane order), the last group merges the groups
  const int ngroups = (nchunks + G - 1) / G, grp = c / G;
  unsigned* ctr = arrive + r * (ngroups + 1);
  const int q0 = grp * G, q1 = q0 + G < nchunks ? q0 + G : nchunks;
  if (!mom_last_arrival(ctr + grp, (unsigned)(q1 - q0))) return;
  double* gpart = part + nrows * nchunks * 5;
  const Mom zero = {0.0, 0.0, 0.0, 0.0, 0.0};
  Mom m = q0 + tid < q1 ? m4_load(part + (r * nchunks + q0 + tid) * 5, 1) : zero;
  m = m4_block_merge(m, sh);
  if (tid == 0) m4_store_wt(gpart + (r * ngroups + grp) * 5, 1, m);
  if (!mom_last_arrival(ctr + ngroups, (unsigned)ngroups)) return;
  m = tid < ngroups ? m4_load(gpart + (r * ngroups + tid) * 5, 1) : zero;
  m = m4_block_merge(m, sh);
  if (tid == 0) m4_store(out + r, nrows, m);
}

// Unsplit rows (nchunks == 1; the caller splits rows beyond 16K elements): a wave per row, four rows
// per workgroup; the row is one segment, so its result needs no LDS and no merge.
template <typename T>
__global__ __launch_bounds__(256) void m4_rows_wave(const T* __restrict__ x, int64_t nrows, int64_t len,
                                                    int64_t ld, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nrows) return;  // wave-uniform
  const T* row = x + r * ld;
  const double K = m4_shift(row, len, lane);
  Pow s = {0.0, 0.0, 0.0, 0.0};
  m4_accum<T, 64>(row, len, lane, K, s);
  s = wave_pow_sum(s);
  if (lane == 0) m4_store(out + r, nrows, m4_from_shifted((double)len, K, s));
}

// One row of a thread's VEC consecutive columns, widened (VEC > 1: one 16-byte load)
template <typename T, int VEC>
__device__ __forceinline__ void m4_ldcols(const T* p, double (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = (double)__builtin_nontemporal_load(p);
  } else {
    const typename Vec16<T>::type a =
        __builtin_nontemporal_load(reinterpret_cast<const typename Vec16<T>::type*>(p));
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = (double)a[e];
  }
}

// columns: x[i * ld + col], reduce over i in [0, len). A thread owns VEC consecutive columns (16
// bytes, or one column when the matrix is not 16-byte tileable) with a shift per column; grid =
// (ceil(ncols / (256 VEC)), nchunks) row chunks. part: planes per slot, field k of column col in
// slot s at ((s * 5 + k) * ncols + col), chunk partials in slots [0, nchunks), group partials
// after them, so partial stores and merge loads are coalesced. out: field k at out[k * ncols + col].
template <typename T, int VEC>
__global__ __launch_bounds__(256) void m4_cols(const T* __restrict__ x, int64_t len, int64_t ncols, int64_t ld,
                                               int nchunks, int G, double* __restrict__ part,
                                               double* __restrict__ out, unsigned* __restrict__ cnt) {
  const int64_t col0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  const int c = blockIdx.y;
  const int64_t per = (len + nchunks - 1) / nchunks;
  const int64_t r0 = (int64_t)c * per;
  const int64_t r1 = r0 + per < len ? r0 + per : len;
  if (col0 < ncols) {  // VEC > 1 only with ncols % VEC == 0: all VEC columns exist
    double K[VEC];
    Pow s[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      K[e] = 0.0;
      s[e] = Pow{0.0, 0.0, 0.0, 0.0};
    }
    const T* base = x + col0;
    if (r0 < r1) {
      const int m = r1 - r0 < 16 ? (int)(r1 - r0) : 16;
      double x0[VEC], acc[VEC], v[VEC];
      m4_ldcols<T, VEC>(base + r0 * ld, x0);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
      for (int i = 1; i < m; ++i) {
        m4_ldcols<T, VEC>(base + (r0 + i) * ld, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += v[e] - x0[e];
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) K[e] = x0[e] + acc[e] / (double)m;
    }
    int64_t i = r0;
    for (; i + 7 < r1; i += 8) {  // 8 rows (128 B per thread) in flight
      double a[8][VEC];
#pragma unroll
      for (int u = 0; u < 8; ++u) m4_ldcols<T, VEC>(base + (i + u) * ld, a[u]);
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) m4_add(s[e], a[u][e], K[e]);
    }
    for (; i < r1; ++i) {
      double a[VEC];
      m4_ldcols<T, VEC>(base + i * ld, a);
#pragma unroll
      for (int e = 0; e < VEC; ++e) m4_add(s[e], a[e], K[e]);
    }
    const double n = (double)(r1 > r0 ? r1 - r0 : 0);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const Mom m = m4_from_shifted(n, K[e], s[e]);
      if (nchunks == 1)
        m4_store(out + col0 + e, ncols, m);
      else
        m4_store_wt(part + (int64_t)c * 5 * ncols + col0 + e, ncols, m);  // to the group's last block
    }
  }
  if (nchunks == 1) return;
  // two-level tree as in mom_cols: a group's last-arriving block merges its chunks in chunk order,
  // the last group merges the groups in group order - the same result whatever the arrival order
  const int ngroups = (nchunks + G - 1) / G, grp = c / G;
  unsigned* ctr = cnt + (int64_t)blockIdx.x * (ngroups + 1);
  const int q0 = grp * G, q1 = q0 + G < nchunks ? q0 + G : nchunks;
  if (!mom_last_arrival(ctr + grp, (unsigned)(q1 - q0))) return;
  double* gpart = part + (int64_t)nchunks * 5 * ncols;
  if (col0 < ncols) {
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      m4_store_wt(gpart + (int64_t)grp * 5 * ncols + col0 + e, ncols,
                  m4_merge_strided(part + col0 + e, q0, q1, 5 * ncols, ncols));
  }
  if (!mom_last_arrival(ctr + ngroups, (unsigned)ngroups)) return;
  if (col0 >= ncols) return;
#pragma unroll
  for (int e = 0; e < VEC; ++e)
    m4_store(out + col0 + e, ncols, m4_merge_strided(gpart + col0 + e, 0, ngroups, 5 * ncols, ncols));
}

// Chunks per merge group (ceil(sqrt(nchunks)): both tree levels short)
int m4_group(int nchunks) {
  int g = 1;
  while (g * g < nchunks) ++g;
  return g;
}

template <typename T>
int m4_launch_rows(const T* x, int64_t nrows, int64_t len, int64_t ld, int nchunks, double* part, double* out,
                   unsigned* cnt, hipStream_t stream) {
  if (nchunks == 1) {
    const int64_t blocks = (nrows + 3) / 4;
    if (blocks > 0x7fffffffLL) return HA_UNSUPPORTED;
    hipLaunchKernelGGL(m4_rows_wave<T>, dim3((unsigned)blocks), dim3(256), 0, stream, x, nrows, len, ld, out);
    return ha_launch_status();
  }
  const int64_t grid = nrows * nchunks;
  if (grid > 0x7fffffffLL) return HA_UNSUPPORTED;
  hipLaunchKernelGGL(m4_rows<T>, dim3((unsigned)grid), dim3(256), 0, stream, x, nrows, len, ld, nchunks,
                     m4_group(nchunks), part, out, cnt);
  return ha_launch_status();
}

template <typename T>
int m4_launch_cols(const T* x, int64_t len, int64_t ncols, int64_t ld, int nchunks, double* part, double* out,
                   unsigned* cnt, hipStream_t stream) {
  constexpr int E = Vec16<T>::N;
  const bool vec = (ncols % E == 0) && (ld % E == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  const int64_t gx = ((vec ? ncols / E : ncols) + 255) / 256;
  if (gx > 0x7fffffffLL) return HA_UNSUPPORTED;
  if (vec)
    hipLaunchKernelGGL((m4_cols<T, E>), dim3((unsigned)gx, nchunks), dim3(256), 0, stream, x, len, ncols, ld,
                       nchunks, m4_group(nchunks), part, out, cnt);
  else
    hipLaunchKernelGGL((m4_cols<T, 1>), dim3((unsigned)gx, nchunks), dim3(256), 0, stream, x, len, ncols, ld,
                       nchunks, m4_group(nchunks), part, out, cnt);
  return ha_launch_status();
}

}  // namespace

// Workspace of ha_moments4_rows: doubles of part, arrival counters (zeroed; the kernel resets them)
HA_EXPORT void ha_moments4_rows_workspace(int64_t nrows, int nchunks, int64_t* part_doubles, int64_t* counters) {
  const int g = m4_group(nchunks > 0 ? nchunks : 1);
  const int64_t ngroups = (nchunks + g - 1) / g;
  *part_doubles = nchunks > 1 ? nrows * (nchunks + ngroups) * 5 : 0;
  *counters = nchunks > 1 ? nrows * (ngroups + 1) : 0;
}

// (n, mean, M2, M3, M4) of each row x[r * ld + i], i < len (len >= 1), of element type dtype (0
// float, 1 double), as five planes of nrows doubles in out. nchunks > 1 splits every row over that
// many blocks; part / cnt as ha_moments4_rows_workspace says.
HA_EXPORT int ha_moments4_rows(const void* x, int dtype, int64_t nrows, int64_t len, int64_t ld, int nchunks,
                               double* part, double* out, unsigned* cnt, void* stream) {
  if (nrows <= 0) return HA_OK;
  if (len < 1 || nchunks < 1 || nchunks > 65536 || out == nullptr || (dtype != 0 && dtype != 1) ||
      (nchunks > 1 && (cnt == nullptr || part == nullptr)) ||
      reinterpret_cast<uintptr_t>(x) % (dtype ? sizeof(double) : sizeof(float)) != 0)
    return HA_BAD_ARG;
  if (dtype == 0)
    return m4_launch_rows(static_cast<const float*>(x), nrows, len, ld, nchunks, part, out, cnt, (hipStream_t)stream);
  return m4_launch_rows(static_cast<const double*>(x), nrows, len, ld, nchunks, part, out, cnt, (hipStream_t)stream);
}

// Workspace of ha_moments4_cols: doubles of part, arrival counters
HA_EXPORT void ha_moments4_cols_workspace(int64_t ncols, int nchunks, int64_t* part_doubles, int64_t* counters) {
  const int g = m4_group(nchunks > 0 ? nchunks : 1);
  const int64_t ngroups = (nchunks + g - 1) / g;
  *part_doubles = nchunks > 1 ? (nchunks + ngroups) * 5 * ncols : 0;
  *counters = nchunks > 1 ? ((ncols + 255) / 256) * (ngroups + 1) : 0;
}

// (n, mean, M2, M3, M4) of each column x[i * ld + col], i < len (len >= 1), as five planes of ncols
// doubles in out; dtype, nchunks, part and cnt as for the rows.
HA_EXPORT int ha_moments4_cols(const void* x, int dtype, int64_t len, int64_t ncols, int64_t ld, int nchunks,
                               double* part, double* out, unsigned* cnt, void* stream) {
  if (ncols <= 0) return HA_OK;
  if (len < 1 || nchunks < 1 || nchunks > 65535 || out == nullptr || (dtype != 0 && dtype != 1) ||
      (nchunks > 1 && (cnt == nullptr || part == nullptr)) ||
      reinterpret_cast<uintptr_t>(x) % (dtype ? sizeof(double) : sizeof(float)) != 0)
    return HA_BAD_ARG;
  if (dtype == 0)
    return m4_launch_cols(static_cast<const float*>(x), len, ncols, ld, nchunks, part, out, cnt, (hipStream_t)stream);
  return m4_launch_cols(static_cast<const double*>(x), len, ncols, ld, nchunks, part, out, cnt, (hipStream_t)stream);
}
