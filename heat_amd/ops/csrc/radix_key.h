// Bit-ordered integer keys of float32 / float64 and the 16-byte row load, shared by the selection
// kernels (kmedians.hip, quantile.hip).
#pragma once
#include "common.h"

typedef double rk_doublex2 __attribute__((ext_vector_type(2)));

template <typename T> struct Tr;
template <> struct Tr<float> {
  typedef floatx4 vec;
  typedef int S;        // bit-ordered key
  typedef unsigned U;   // key distance
  static constexpr int V = 4, BITS = 32;
};
template <> struct Tr<double> {
  typedef rk_doublex2 vec;
  typedef long long S;
  typedef unsigned long long U;
  static constexpr int V = 2, BITS = 64;
};

// Keys: the monotone bit map of cluster/_kcluster.py (x < y <=> key(x) < key(y) as signed integers;
// +-0 and NaN patterns order by their bits).
template <typename T>
__device__ __forceinline__ typename Tr<T>::S key_of(T x) {
  typedef typename Tr<T>::S S;
  const S i = __builtin_bit_cast(S, x);
  return i ^ ((i >> (Tr<T>::BITS - 1)) & ~((S)1 << (Tr<T>::BITS - 1)));
}
template <typename T>
__device__ __forceinline__ T value_of(typename Tr<T>::S s) {
  typedef typename Tr<T>::S S;
  return __builtin_bit_cast(T, (S)(s ^ ((s >> (Tr<T>::BITS - 1)) & ~((S)1 << (Tr<T>::BITS - 1)))));
}

// 16 bytes of a row starting at feature col (zeros past f and past the last row): one 16-byte
// non-temporal load where the row is 16-byte aligned and the vector lies inside it, element loads
// otherwise (odd f, unaligned views; a row is never read past its f features).
template <typename T>
__device__ __forceinline__ typename Tr<T>::vec ld_row(const T* __restrict__ base, int64_t row, int64_t nrows,
                                                      int64_t ld, int col, int f, int vec_ok) {
  typedef typename Tr<T>::vec vec;
  constexpr int V = Tr<T>::V;
  vec v = (vec)((T)0);
  if (row < nrows && col < f) {
    const T* p = base + row * ld + col;
    if (vec_ok && col + V <= f) {
      v = __builtin_nontemporal_load(reinterpret_cast<const vec*>(p));
    } else {
#pragma unroll
      for (int q = 0; q < V; ++q)
        if (col + q < f) v[q] = p[q];
    }
  }
  return v;
}
