// hipcc-flags: -fno-slp-vectorize
// Gaussian naive Bayes on CDNA4 (reference heat/naive_bayes/gaussianNB.py: __update_mean_variance 131,
// __joint_log_likelihood 391), for float and double input: the class-conditional moments of the fit
// (ha_gnb_moments, behind ops.class_moments) and the fused likelihood of the predict side (ha_gnb_jll,
// behind ops.gnb_jll). Both read X once; neither makes a float64 copy, an m x f or an m x k x f
// temporary, and neither uses atomics, so results are bit-identical run to run.
//
// (a) gnb_moments: (W, mean, M2) per class and feature as a weighted one-hot product on
//     v_mfma_f64_16x16x4_f64.
//   * A side: 16 classes x 4 rows, w_i where row i has that class and zero elsewhere (lane: class =
//     lane & 15, row = lane >> 4, built from the row's int64 index by one compare per class tile).
//     B side: 4 rows x 16 features of the shifted values d = x - s, and in a second instruction d^2; a
//     third with B = 1 gives the class weights W. A wave keeps sum w d and sum w d^2 of 16 classes x 16
//     features in 8 accumulator doubles per lane, times NB feature blocks, times CT class tiles
//     (16 < k <= 64 walks the class tiles over the rows already in registers, X is not read again).
//   * A lane's B values are its own NB-element row load (16 bytes; 8 bytes for float with 4 class
//     tiles, where 4 blocks would need 256 accumulator registers): block j takes element j, so block
//     j's column c is feature NB c + j of the wave's 16 NB features. Rows or bases that are not
//     NB-aligned take element loads (block j's column c = feature c + 16 j). Float is widened in
//     registers. The next batch of rows (4 U) is loaded before the current one is multiplied.
//   * The shift s is the chunk's first row, one value per feature, the same in every lane that holds the
//     feature: a common offset of 1e4 at unit spread costs nothing. Constant columns give d = 0,
//     mean = s and M2 = 0 exactly.
//   * One wave per workgroup and per (feature group, row chunk); a chunk converts once to
//     (W, s + S1 / W, S2 - S1^2 / W), a class that is absent from it to (0, 0, 0). Chunk triples are
//     merged with Chan's formula in chunk order by two small launches (groups of ceil(sqrt(chunks))
//     chunks, then the groups), as kmeans_smallk.hip finishes its sums: no hand-off between workgroups.
//   * The product adds 0 * d for the other classes: a NaN or infinity in one row reaches every class
//     of that feature (the index_add path keeps it to the row's class). Weights are non-negative.
//   * Instruction budget: per 4 rows x 16 NB features a wave issues CT (2 NB + 1) MFMAs. For float
//     input with k <= 16 that is 9 per KB of X against 5 per KB for double; measurements are in
//     profiles/README.md.
//
// (b) gnb_jll: jll(i, c) = cst(c) - 0.5 sum_f (x(i, f) - theta(c, f))^2 inv(c, f) in the input's
//     precision and in the difference form (a sigma of 1e-9 of the largest makes the expanded form
//     cancel), cst(c) = log_prior(c) - 0.5 sum_f log(2 pi sigma(c, f)).
//   * gnb_prepare (one wave per class) writes theta and 1 / sigma padded to whole feature chunks
//     (padding: theta = 0, inv = 0, which adds exactly 0) and cst, its log sum in double.
//   * One wave per 64 rows, a lane per row. A feature chunk is one 128-byte line per lane (8 loads of 16
//     bytes, non-temporal, the next chunk's in flight before this one is used), so no line is fetched
//     twice whatever the cache keeps. The class loop is uniform: theta and inv of the chunk are scalar
//     operands, the running quadratic form of (class, row) lives in LDS at [class][lane] (one read
//     and one write per chunk and class, conflict-free).
//   * Epilogue per row in registers / LDS: the argmax (strict >, so ties go to the lowest class), or
//     max and sum of exponentials for jll - logsumexp(jll); the [rows, k] tile is then stored
//     coalesced from LDS.
#include "common.h"

namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

template <typename T, int N> struct GVec {
  typedef T type __attribute__((ext_vector_type(N)));
};

// A lane's NB values of one row of a feature group: p = the row's first feature of the group, c =
// lane & 15, left = features from p to the row's end. Features past the end read as 0.
template <typename T, int NB, bool VEC>
__device__ __forceinline__ void gm_load(const T* p, int c, int left, T (&v)[NB]) {
  if constexpr (VEC) {  // left % NB == 0: the vector is inside the row or outside it
    typedef typename GVec<T, NB>::type V;
    if (NB * c < left) {
      const V a = __builtin_nontemporal_load(reinterpret_cast<const V*>(p + NB * c));
#pragma unroll
      for (int j = 0; j < NB; ++j) v[j] = a[j];
    } else {
#pragma unroll
      for (int j = 0; j < NB; ++j) v[j] = T(0);
    }
  } else {
#pragma unroll
    for (int j = 0; j < NB; ++j) v[j] = c + 16 * j < left ? __builtin_nontemporal_load(p + c + 16 * j) : T(0);
  }
}

template <typename T, int NB, int U> struct GmBatch {
  T x[U][NB];
  long long id[U];
  double w[U];
};

// grid = (feature groups of 16 NB, row chunks), 64 threads. Chunk q owns rows [q per, min(m, (q + 1) per)).
// dst: triples as planes, field t of (class, feature) at dst[(slot 3 + t) k f + class f + feature], the
// chunk's slot = q (out itself when there is one chunk).
template <typename T, int NB, int CT, bool VEC>
__global__ __launch_bounds__(64) void gnb_moments(const T* __restrict__ x, int64_t m, int f, int64_t ld,
                                                  const long long* __restrict__ idx, const double* __restrict__ w,
                                                  int k, int64_t per, double* __restrict__ dst) {
  constexpr int U = CT == 1 ? 8 : 4;  // k-steps (4 rows each) per batch; two batches live
  const int lane = threadIdx.x, c = lane & 15, kk = lane >> 4;
  const int f0 = blockIdx.x * 16 * NB, left = f - f0;
  const int64_t r0 = (int64_t)blockIdx.y * per;
  const int64_t r1 = r0 + per < m ? r0 + per : m;
  const T* xb = x + f0;

  double s[NB];
  {
    T sv[NB];
    gm_load<T, NB, VEC>(xb + r0 * ld, c, r0 < r1 ? left : 0, sv);
#pragma unroll
    for (int j = 0; j < NB; ++j) s[j] = (double)sv[j];
  }
  const doublex4 zero = {0.0, 0.0, 0.0, 0.0};
  doublex4 cn[CT], s1[CT][NB], s2[CT][NB];
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    cn[t] = zero;
#pragma unroll
    for (int j = 0; j < NB; ++j) s1[t][j] = s2[t][j] = zero;
  }

  typedef GmBatch<T, NB, U> Batch;
  auto load = [&](int64_t r, Batch& b) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = r + 4 * u + kk;
      const bool in = row < r1;
      b.id[u] = in ? idx[row] : -1;
      b.w[u] = in ? (w ? w[row] : 1.0) : 0.0;
      gm_load<T, NB, VEC>(xb + row * ld, c, in ? left : 0, b.x[u]);
    }
  };

  Batch cur;
  load(r0, cur);
  for (int64_t r = r0; r < r1; r += 4 * U) {
    Batch nxt;
    load(r + 4 * U, nxt);  // past the chunk: nothing is read
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = cur.id[u] >= 0;
      double d[NB], d2[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        d[j] = in ? (double)cur.x[u][j] - s[j] : 0.0;
        d2[j] = d[j] * d[j];
      }
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        const double a = cur.id[u] == (long long)(16 * t + c) ? cur.w[u] : 0.0;
        cn[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, 1.0, cn[t], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          s1[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, d[j], s1[t][j], 0, 0, 0);
          s2[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, d2[j], s2[t][j], 0, 0, 0);
        }
      }
    }
    cur = nxt;
  }

  // C/D map: column = lane & 15, row = (lane >> 4) + 4 reg
  const int64_t kf = (int64_t)k * f;
  double* o = dst + (gridDim.y > 1 ? (int64_t)blockIdx.y * 3 * kf : 0);
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cls = 16 * t + kk + 4 * g;
      if (cls >= k) continue;
      const double W = cn[t][g];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int fe = VEC ? NB * c + j : c + 16 * j;
        if (fe >= left) continue;
        double n = 0.0, mean = 0.0, m2 = 0.0;
        if (!(W == 0.0)) {
          const double dl = s1[t][j][g] / W;
          n = W;
          mean = s[j] + dl;
          m2 = s2[t][j][g] - s1[t][j][g] * dl;
          if (m2 < 0) m2 = 0.0;  // rounding; a NaN passes
        }
        double* p = o + (int64_t)cls * f + f0 + fe;
        p[0] = n;
        p[kf] = mean;
        p[2 * kf] = m2;
      }
    }
}

// Chan merge, in slot order, of the triples in slots [g G, min(nin, (g + 1) G)) of `in` into slot g of
// `out`, g = blockIdx.y; a thread per (class, feature). Empty triples (W = 0) add nothing.
__global__ __launch_bounds__(256) void gnb_merge(const double* __restrict__ in, int nin, int G, int64_t kf,
                                                 double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= kf) return;
  const int g = blockIdx.y;
  const int q0 = g * G, q1 = q0 + G < nin ? q0 + G : nin;
  double n = 0.0, mu = 0.0, m2 = 0.0;
  for (int q = q0; q < q1; ++q) {
    const double* p = in + (int64_t)q * 3 * kf + e;
    const double bn = p[0], bm = p[kf], b2 = p[2 * kf];
    if (bn == 0.0) continue;
    if (n == 0.0) {
      n = bn;
      mu = bm;
      m2 = b2;
    } else {
      const double tot = n + bn, d = bm - mu;
      mu += d * (bn / tot);
      m2 += b2 + d * d * (n * bn / tot);
      n = tot;
    }
  }
  double* o = out + (int64_t)g * 3 * kf + e;
  o[0] = n;
  o[kf] = mu;
  o[2 * kf] = m2;
}

int gm_group(int nchunks) {
  int g = 1;
  while (g * g < nchunks) ++g;
  return g;
}

int gm_tiles(int k) { return k <= 16 ? 1 : (k <= 32 ? 2 : 4); }

// feature blocks per wave: 16 bytes per lane and row, 8 for float with 4 class tiles
int gm_blocks(int dtype, int k) { return dtype == 1 || gm_tiles(k) == 4 ? 2 : 4; }

template <typename T, int NB, int CT>
int gm_launch(const T* x, int64_t m, int f, int64_t ld, const long long* idx, const double* w, int k, int nchunks,
              int64_t per, double* dst, hipStream_t stream) {
  const bool vec = f % NB == 0 && ld % NB == 0 && reinterpret_cast<uintptr_t>(x) % (NB * sizeof(T)) == 0;
  const dim3 grid((unsigned)((f + 16 * NB - 1) / (16 * NB)), (unsigned)nchunks);
  if (vec)
    hipLaunchKernelGGL((gnb_moments<T, NB, CT, true>), grid, dim3(64), 0, stream, x, m, f, ld, idx, w, k, per, dst);
  else
    hipLaunchKernelGGL((gnb_moments<T, NB, CT, false>), grid, dim3(64), 0, stream, x, m, f, ld, idx, w, k, per, dst);
  return ha_launch_status();
}

template <typename T, int NB>
int gm_launch_ct(const T* x, int64_t m, int f, int64_t ld, const long long* idx, const double* w, int k, int nchunks,
                 int64_t per, double* dst, hipStream_t stream) {
  switch (gm_tiles(k)) {
    case 1: return gm_launch<T, NB, 1>(x, m, f, ld, idx, w, k, nchunks, per, dst, stream);
    case 2: return gm_launch<T, NB, 2>(x, m, f, ld, idx, w, k, nchunks, per, dst, stream);
    default:
      if constexpr (NB * sizeof(T) == 16 && sizeof(T) == 4)
        return HA_UNSUPPORTED;  // float with 4 class tiles runs on 2 blocks (gm_blocks)
      else
        return gm_launch<T, NB, 4>(x, m, f, ld, idx, w, k, nchunks, per, dst, stream);
  }
}

// ------------------------------------------------------------------------------------------ likelihood
template <typename T> struct Jll {
  static constexpr int E = 16 / sizeof(T);    // elements per load
  static constexpr int FC = 128 / sizeof(T);  // features per chunk: one 128-byte line per lane
};

// One wave per class c: thp / inv [k][fpad] (zero past f), cst[k].
template <typename T>
__global__ __launch_bounds__(64) void gnb_prepare(const T* __restrict__ theta, int64_t ldt, const T* __restrict__ sigma,
                                                  int64_t lds, const T* __restrict__ lp, int f, int fpad,
                                                  T* __restrict__ thp, T* __restrict__ inv, T* __restrict__ cst) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double acc = 0.0;
  for (int j = lane; j < fpad; j += 64) {
    T th = T(0), iv = T(0);
    if (j < f) {
      const T sg = sigma[c * lds + j];
      th = theta[c * ldt + j];
      iv = T(1) / sg;
      acc += log(6.283185307179586476925 * (double)sg);
    }
    thp[(int64_t)c * fpad + j] = th;
    inv[(int64_t)c * fpad + j] = iv;
  }
  acc = ha_wave_sum_d(acc);
  if (lane == 0) cst[c] = (T)((double)lp[c] - 0.5 * acc);
}

// grid = ceil(m / 64), 64 threads, k * 64 * sizeof(T) bytes of LDS. mode 0: out[m, k] = jll; 1: lab[m] =
// argmax; 2: out[m, k] = jll - logsumexp(jll).
template <typename T, bool VEC>
__global__ __launch_bounds__(64) void gnb_jll(const T* __restrict__ x, int64_t m, int f, int64_t ld,
                                              const T* __restrict__ thp, const T* __restrict__ inv,
                                              const T* __restrict__ cst, int k, int fpad, int mode,
                                              T* __restrict__ out, long long* __restrict__ lab) {
  constexpr int E = Jll<T>::E, FC = Jll<T>::FC;
  typedef typename GVec<T, E>::type V;
  extern __shared__ __attribute__((aligned(16))) unsigned char gnb_smem[];
  T* jl = reinterpret_cast<T*>(gnb_smem);  // [k][64]
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * 64, row = row0 + lane;
  const bool live = row < m;
  const T* xr = x + (live ? row : row0) * ld;

  auto load = [&](int j0, T(&v)[FC]) {
    if constexpr (VEC) {  // f % E == 0: a vector is inside the row or outside it
#pragma unroll
      for (int u = 0; u < FC / E; ++u) {
        const int j = j0 + E * u;
        V a;
#pragma unroll
        for (int e = 0; e < E; ++e) a[e] = T(0);
        if (live && j < f) a = __builtin_nontemporal_load(reinterpret_cast<const V*>(xr + j));
#pragma unroll
        for (int e = 0; e < E; ++e) v[E * u + e] = a[e];
      }
    } else {
#pragma unroll
      for (int j = 0; j < FC; ++j) v[j] = live && j0 + j < f ? __builtin_nontemporal_load(xr + j0 + j) : T(0);
    }
  };

  T cur[FC];
  load(0, cur);
  for (int j0 = 0; j0 < fpad; j0 += FC) {
    T nxt[FC];
    load(j0 + FC, nxt);  // past the row: nothing is read
    for (int c = 0; c < k; ++c) {
      const T* tp = thp + (int64_t)c * fpad + j0;
      const T* ip = inv + (int64_t)c * fpad + j0;
      T q = j0 ? jl[c * 64 + lane] : T(0);
#pragma unroll
      for (int j = 0; j < FC; ++j) {
        const T d = cur[j] - tp[j];
        q = fma(d * d, ip[j], q);
      }
      jl[c * 64 + lane] = q;
    }
#pragma unroll
    for (int j = 0; j < FC; ++j) cur[j] = nxt[j];
  }

  T best = T(0);
  long long bc = 0;
  for (int c = 0; c < k; ++c) {
    const T v = cst[c] - T(0.5) * jl[c * 64 + lane];
    jl[c * 64 + lane] = v;
    if (c == 0 || v > best) {
      best = v;
      bc = c;
    }
  }
  if (mode == 1) {
    if (live) lab[row] = bc;
    return;
  }
  if (mode == 2) {
    T sum = T(0);
    for (int c = 0; c < k; ++c) sum += exp(jl[c * 64 + lane] - best);
    const T lse = best + log(sum);
    for (int c = 0; c < k; ++c) jl[c * 64 + lane] -= lse;
  }
  __syncthreads();
  const int64_t rest = m - row0;
  const int total = (int)(rest < 64 ? rest : 64) * k;
  T* o = out + row0 * k;
  for (int e = lane; e < total; e += 64) {
    const int r = e / k;
    o[e] = jl[(e - r * k) * 64 + r];
  }
}

template <typename T>
int jll_launch(const T* x, int64_t m, int f, int64_t ld, const T* theta, int64_t ldt, const T* sigma, int64_t lds,
               const T* lp, int k, int mode, T* work, void* out, hipStream_t stream) {
  constexpr int E = Jll<T>::E, FC = Jll<T>::FC;
  const int fpad = (f + FC - 1) / FC * FC;
  T* thp = work;
  T* inv = work + (int64_t)k * fpad;
  T* cst = inv + (int64_t)k * fpad;
  hipLaunchKernelGGL(gnb_prepare<T>, dim3(k), dim3(64), 0, stream, theta, ldt, sigma, lds, lp, f, fpad, thp, inv,
                     cst);
  const int64_t blocks = (m + 63) / 64;
  if (blocks > 0x7fffffffLL) return HA_UNSUPPORTED;
  const bool vec = f % E == 0 && ld % E == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
  const size_t lds_bytes = (size_t)k * 64 * sizeof(T);
  T* o = mode == 1 ? nullptr : static_cast<T*>(out);
  long long* lab = mode == 1 ? static_cast<long long*>(out) : nullptr;
  if (vec)
    hipLaunchKernelGGL((gnb_jll<T, true>), dim3((unsigned)blocks), dim3(64), lds_bytes, stream, x, m, f, ld, thp, inv,
                       cst, k, fpad, mode, o, lab);
  else
    hipLaunchKernelGGL((gnb_jll<T, false>), dim3((unsigned)blocks), dim3(64), lds_bytes, stream, x, m, f, ld, thp,
                       inv, cst, k, fpad, mode, o, lab);
  return ha_launch_status();
}

}  // namespace

// Row chunks of ha_gnb_moments for m rows, f features, k classes of dtype (0 float, 1 double) on ncu
// compute units: about 8 waves per CU over the feature groups, and chunks of at least max(512, 128 k)
// rows, so that a chunk's 3 k triples per feature stay under 5% of the bytes it reads.
HA_EXPORT int ha_gnb_moments_chunks(int64_t m, int f, int k, int dtype, int ncu) {
  if (m < 1 || f < 1 || k < 1 || k > 64 || ncu < 1) return 1;
  const int fb = 16 * gm_blocks(dtype, k);
  const int64_t groups = (f + fb - 1) / fb;
  const int64_t min_rows = k * 128 > 512 ? k * 128 : 512;
  int64_t n = (8LL * ncu + groups - 1) / groups;
  if (n > (m + min_rows - 1) / min_rows) n = (m + min_rows - 1) / min_rows;
  if (n > 65535) n = 65535;
  if (n < 1) n = 1;
  const int64_t per = (m + n - 1) / n;
  return (int)((m + per - 1) / per);  // no empty chunk
}

// Doubles of ha_gnb_moments' `part` for nchunks chunks (0 for one chunk)
HA_EXPORT int64_t ha_gnb_moments_workspace(int nchunks, int k, int f) {
  if (nchunks <= 1) return 0;
  const int g = gm_group(nchunks);
  return (int64_t)(nchunks + (nchunks + g - 1) / g) * 3 * k * f;
}

// (W, mean, M2) of every class and feature of x[m, f] (row stride ld, dtype 0 float / 1 double): row i
// counts with weight w[i] (1 if w is null) for class idx[i]; rows whose index is outside [0, k) count for
// no class. out: three planes of k x f doubles, W repeated along the features. 1 <= k <= 64;
// nchunks from ha_gnb_moments_chunks (any value in [1, min(m, 65535)] is served), part as
// ha_gnb_moments_workspace says.
HA_EXPORT int ha_gnb_moments(const void* x, int dtype, int64_t m, int f, int64_t ld, const void* idx, const double* w,
                             int k, int nchunks, double* part, double* out, void* stream) {
  if (m < 1 || f < 1 || k < 1 || k > 64 || nchunks < 1 || nchunks > 65535 || nchunks > m || x == nullptr ||
      idx == nullptr || out == nullptr || (dtype != 0 && dtype != 1) || (nchunks > 1 && part == nullptr) ||
      reinterpret_cast<uintptr_t>(x) % (dtype ? sizeof(double) : sizeof(float)) != 0 ||
      reinterpret_cast<uintptr_t>(idx) % 8 != 0)
    return HA_BAD_ARG;
  const int64_t per = (m + nchunks - 1) / nchunks;
  if ((int64_t)(nchunks - 1) * per >= m) return HA_BAD_ARG;  // an empty last chunk
  hipStream_t s = (hipStream_t)stream;
  const long long* id = static_cast<const long long*>(idx);
  double* dst = nchunks > 1 ? part : out;
  int rc;
  if (dtype == 1)
    rc = gm_launch_ct<double, 2>(static_cast<const double*>(x), m, f, ld, id, w, k, nchunks, per, dst, s);
  else if (gm_blocks(0, k) == 4)
    rc = gm_launch_ct<float, 4>(static_cast<const float*>(x), m, f, ld, id, w, k, nchunks, per, dst, s);
  else
    rc = gm_launch<float, 2, 4>(static_cast<const float*>(x), m, f, ld, id, w, k, nchunks, per, dst, s);
  if (rc != HA_OK || nchunks == 1) return rc;
  const int64_t kf = (int64_t)k * f;
  const int G = gm_group(nchunks), ng = (nchunks + G - 1) / G;
  const unsigned gx = (unsigned)((kf + 255) / 256);
  double* gpart = part + (int64_t)nchunks * 3 * kf;
  hipLaunchKernelGGL(gnb_merge, dim3(gx, ng), dim3(256), 0, s, (const double*)part, nchunks, G, kf, gpart);
  hipLaunchKernelGGL(gnb_merge, dim3(gx, 1), dim3(256), 0, s, (const double*)gpart, ng, ng, kf, out);
  return ha_launch_status();
}

// Elements (of x's type) of ha_gnb_jll's `work`: theta and 1 / sigma padded to whole chunks, and cst
HA_EXPORT int64_t ha_gnb_jll_work(int k, int f, int dtype) {
  const int fc = dtype ? Jll<double>::FC : Jll<float>::FC;
  return (int64_t)k * ((f + fc - 1) / fc * fc) * 2 + k;
}

// Joint log likelihood of x[m, f] (row stride ld, dtype 0 float / 1 double) under k <= 64 classes with
// theta / sigma [k, f] (row strides ldt / lds) and log_prior lp[k], all of x's type. mode 0: out[m, k] of
// x's type; 1: out = int64 labels [m], ties to the lowest class; 2: out[m, k] = jll - logsumexp(jll).
HA_EXPORT int ha_gnb_jll(const void* x, int dtype, int64_t m, int f, int64_t ld, const void* theta, int64_t ldt,
                         const void* sigma, int64_t lds, const void* lp, int k, int mode, void* work, void* out,
                         void* stream) {
  const size_t es = dtype ? sizeof(double) : sizeof(float);
  if (m < 1 || f < 1 || k < 1 || k > 64 || mode < 0 || mode > 2 || (dtype != 0 && dtype != 1) || x == nullptr ||
      theta == nullptr || sigma == nullptr || lp == nullptr || work == nullptr || out == nullptr ||
      reinterpret_cast<uintptr_t>(x) % es != 0 || reinterpret_cast<uintptr_t>(work) % es != 0 ||
      reinterpret_cast<uintptr_t>(out) % (mode == 1 ? 8 : es) != 0)
    return HA_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 1)
    return jll_launch(static_cast<const double*>(x), m, f, ld, static_cast<const double*>(theta), ldt,
                      static_cast<const double*>(sigma), lds, static_cast<const double*>(lp), k, mode,
                      static_cast<double*>(work), out, s);
  return jll_launch(static_cast<const float*>(x), m, f, ld, static_cast<const float*>(theta), ldt,
                    static_cast<const float*>(sigma), lds, static_cast<const float*>(lp), k, mode,
                    static_cast<float*>(work), out, s);
}
