// Host-side AddressSanitizer check of the native library's C ABI (sanitizer builds
// of the native extension). Built by tests/test_asan_host.py against an ASan-instrumented copy of
// the library (-fsanitize=address on the HOST code only: GPU ASan is not available here). Calls
// every host-only entry point (workspace / capacity calculators) over many shapes and the launch
// wrappers with arguments they must reject before touching the GPU, so ASan sees all host paths
// that run without a device. Prints "asan host check ok" and exits 0 on success.
#include <dlfcn.h>
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" {
int64_t ha_h3_amb_rows(int64_t n);
int ha_h3_amb_shards();
int ha_h3_fpad(int f);
int64_t ha_h3_workspace_bytes(int k, int f);
void ha_moments_rows_workspace(int64_t nrows, int nchunks, int64_t* part_doubles, int64_t* counters);
void ha_moments_cols_workspace(int64_t ncols, int nchunks, int64_t* part_doubles, int64_t* counters);
int64_t ha_lasso_prepare_scratch(int64_t m, int n);
int64_t ha_lasso_partial_floats(int num_cus);
int64_t ha_hh_part_len(int64_t m);
int ha_hh_counters();
int ha_hh_nb();
int ha_hh_slen();
int64_t ha_km_update_workspace(int64_t n, int k, int f, int num_cus);
int ha_km_workspace_floats(int k, int f, int* fpad_out, int* kpad_out);
int64_t ha_gemm_tiled_slices(int64_t K, int64_t slices);
int ha_moments_rows(const float* x, int64_t nrows, int64_t len, int64_t ld, int nchunks, double* part, void* out,
                    int kind, double ddof, unsigned* cnt, void* stream);
int ha_moments_cols(const float* x, int64_t len, int64_t ncols, int64_t ld, int nchunks, double* part, void* out,
                    int kind, double ddof, unsigned* cnt, void* stream);
int ha_gemm_f32t(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                 int64_t ldc, int a_kmajor, int b_kmajor, float alpha, int beta, int upper, int64_t slices,
                 int64_t cslice, void* stream);
int ha_gemm_h3t(const void* Ahi, const void* Alo, const void* Bhi, const void* Blo, const int* eA, const int* eB,
                float* C, int64_t M, int64_t N, int64_t Kp, int64_t Mp, int64_t Np, int64_t ldc, float alpha, int beta,
                int upper, int64_t slices, int64_t cslice, void* stream);
int ha_hh_colsums(const void* A, int dtype, int64_t m, int64_t lda, int64_t g0, int64_t k0, int ncols, int64_t d,
                  double* S, double* part, unsigned* cnt, void* stream);
int ha_hh_step(void* A, int dtype, int64_t m, int64_t lda, int64_t g0, int64_t k0, int64_t coff, int ncols, int j,
               const double* Sin, double* Sout, void* tau, double* Y, double* part, unsigned* cnt, void* stream);
int ha_threefry_fill(void* out, int64_t e0, int64_t n, uint64_t counter_lo, uint64_t counter_hi, uint64_t seed,
                     int bits, int dist, double low, double span, void* stream);
int ha_knn_rescore(const float* Q, int64_t ldq, const float* T, int64_t ldt, int64_t nt, int64_t nq, int f,
                   const void* cand, int idx64, int c, int k, float* dist, int64_t* out_idx, void* stream);
int64_t ha_km_label_order_workspace(int64_t n, int k);
int64_t ha_km_label_order_cstart(int64_t n, int k);
int ha_km_label_order(const int* labels, int64_t n, int k, int* workspace, void* stream);
int ha_l1_point_block();
int ha_l1_centroid_tile(int k);
int ha_l1_assign(const void* X, int dtype, int64_t n, int f, int64_t ldx, const void* C, int k, int64_t ldc, int* labels,
                 void* mind, void* stream);
int ha_l1_to_label(const void* X, int dtype, int64_t n, int f, int64_t ldx, const void* M, int k, int64_t ldm,
                   const int* labels, void* d, void* stream);
int ha_med_segment();
int64_t ha_med_table_bytes(int k, int f, int64_t cap);
int ha_med_minmax(const void* X, int dtype, int64_t n, int f, int64_t ldx, const int* order, const int* cstart, int k,
                  void* mm, void* stream);
int ha_med_setup(int dtype, const void* mm, const void* counts, int k, int f, void* prefix, void* rank, int* npass,
                 int* maxpass, void* stream);
int ha_med_select(const void* X, int dtype, int64_t n, int f, int64_t ldx, const int* order, const int* cstart, int k,
                  const void* mm, const void* prefix, const int* npass, int pass, void* table, int64_t table_bytes,
                  void* stream);
int ha_med_pick(int dtype, int k, int f, int pass, void* table, int64_t table_bytes, void* prefix, void* rank,
                const int* npass, void* stream);
int ha_med_fixup(const void* X, int dtype, int64_t n, int f, int64_t ldx, const int* order, const int* cstart, int k,
                 const void* mm, const void* prefix, void* fx, void* stream);
int ha_med_finish(int dtype, int k, int f, const void* mm, const void* prefix, const void* counts, const void* fx,
                  void* med, void* stream);
int ha_qsel_max_targets();
int ha_qsel_group();
int ha_qsel_passes(int dtype, int layout);
int ha_qsel_small_len(int dtype);
int64_t ha_qsel_table_elems(int layout, int64_t slices, int R, int pass, int64_t cap);
int ha_qsel_rows_small(const void* x, int dtype, int64_t nrows, int64_t len, int64_t ld, const void* ranks, int R,
                       void* out, void* stream);
int ha_qsel_rows_pass(const void* src, int dtype, int layout, int mode, int64_t slices, int64_t len, int64_t ld,
                      int nchunks, int pass, int R, int t0, int tg, int append, const void* prefix, const void* live,
                      void* table, int64_t table_elems, void* comp, void* ccnt, int64_t ccap, void* stream);
int ha_qsel_cols_pass(const void* X, int dtype, int64_t n, int64_t ncols, int64_t ld, int nchunks, int pass, int R,
                      int t0, int tg, int append, const void* prefix, const void* live, void* table,
                      int64_t table_elems, void* comp, void* ccnt, int64_t ccap, void* stream);
int ha_qsel_pick(int dtype, int layout, int64_t slices, int R, int pass, const void* ranks, const void* table,
                 int64_t table_elems, void* prefix, void* rank, void* cnt, void* live, void* key, void* nan,
                 void* record, void* stream);
int ha_qsel_finish(int dtype, int64_t slices, int R, const void* key, const void* nan, void* out, void* stream);
}

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "check failed line %d: %s\n", __LINE__, #c); \
      ++fails;                                                    \
    }                                                             \
  } while (0)

int main() {
  enum { OK = 0, BAD = 1, UNSUP = 2 };
  const int64_t sizes[] = {0, 1, 3, 255, 256, 257, 4096, 12500000, 100000007};
  for (int64_t n : sizes) {
    const int64_t r = ha_h3_amb_rows(n);
    CHECK(r >= n && r % ha_h3_amb_shards() == 0);
    CHECK(ha_hh_part_len(n > 0 ? n : 1) % ha_hh_nb() == 0);
    for (int k : {1, 7, 64, 1024})
      for (int f : {3, 16, 64})
        if (n < ((int64_t)1 << 31)) CHECK(ha_km_update_workspace(n, k, f, 256) >= 0);
  }
  for (int nchunks : {1, 2, 17, 4096, 65536}) {
    int64_t pd = -1, nc = -1;
    ha_moments_rows_workspace(5, nchunks, &pd, &nc);
    CHECK(pd >= 15 && nc >= 0);
    ha_moments_cols_workspace(1000, nchunks, &pd, &nc);
    CHECK(pd >= 3000 && nc >= 4);
  }
  for (int f : {1, 16, 17, 64, 100, 128, 129}) {
    const int fp = ha_h3_fpad(f);
    CHECK(fp == -1 || fp >= f);
    if (fp > 0) CHECK(ha_h3_workspace_bytes(1024, f) > 0);
    int fpad = 0, kpad = 0;
    const int w = ha_km_workspace_floats(1000, f, &fpad, &kpad);
    CHECK(w < 0 || (fpad >= f && kpad >= 1000));
  }
  for (int64_t m : {1, 1000, 10000000}) CHECK(ha_lasso_prepare_scratch(m, 16) >= 16);
  CHECK(ha_lasso_partial_floats(256) >= 4 + 1024);
  CHECK(ha_hh_slen() == ha_hh_counters() * 2 * ha_hh_nb());
  for (int64_t K : {1, 16, 17, 4096, 1250000})
    for (int64_t s : {1, 2, 7, 1000}) {
      const int64_t t = ha_gemm_tiled_slices(K, s);
      CHECK(t >= 1 && t <= s);
    }
  // launch wrappers: invalid arguments are rejected before any device work
  float dummy[16] = {0};
  CHECK(ha_moments_rows(dummy, 4, 100, 100, 0, nullptr, nullptr, 1, 0.0, nullptr, nullptr) == BAD);
  CHECK(ha_moments_rows(dummy, 4, 100, 100, 70000, nullptr, nullptr, 1, 0.0, nullptr, nullptr) == BAD);
  CHECK(ha_moments_rows(dummy, 4, 100, 100, 8, (double*)dummy, dummy, 1, 0.0, nullptr, nullptr) == BAD);
  CHECK(ha_moments_rows(dummy, 0, 100, 100, 8, nullptr, nullptr, 1, 0.0, nullptr, nullptr) == OK);
  CHECK(ha_moments_cols(dummy, 100, 4, 4, 0, nullptr, nullptr, 1, 0.0, nullptr, nullptr) == BAD);
  CHECK(ha_moments_cols(dummy, 100, 0, 4, 4, nullptr, nullptr, 1, 0.0, nullptr, nullptr) == OK);
  CHECK(ha_gemm_f32t(dummy, dummy, dummy, -1, 4, 4, 4, 4, 4, 0, 0, 1.f, 0, 0, 1, 0, nullptr) == BAD);
  CHECK(ha_gemm_f32t(dummy, dummy, dummy, 8, 4, 4, 4, 4, 4, 0, 0, 1.f, 0, 1, 1, 0, nullptr) == BAD);  // upper, M != N
  CHECK(ha_gemm_f32t(dummy, dummy, dummy, 0, 4, 4, 4, 4, 4, 0, 0, 1.f, 0, 0, 1, 0, nullptr) == OK);
  CHECK(ha_gemm_f32t(dummy, dummy, dummy, 4, 4, 2, 4, 4, 4, 0, 0, 1.f, 0, 0, 1, 0, nullptr) == UNSUP);  // K < 4
  CHECK(ha_gemm_h3t(dummy, dummy, dummy, dummy, nullptr, nullptr, dummy, 10, 10, 15, 256, 256, 10, 1.f, 0, 0, 1, 0,
                    nullptr) == BAD);  // Kp % 16
  CHECK(ha_gemm_h3t(dummy, dummy, dummy, dummy, nullptr, nullptr, dummy, 300, 10, 16, 256, 256, 10, 1.f, 0, 0, 1, 0,
                    nullptr) == BAD);  // Mp < M
  CHECK(ha_hh_colsums(dummy, 0, 10, 4, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr) == BAD);
  CHECK(ha_hh_colsums(dummy, 0, 10, 4, 0, 0, 99, 0, nullptr, nullptr, nullptr, nullptr) == BAD);
  CHECK(ha_hh_step(dummy, 0, 10, 4, 0, 0, 0, 4, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
        BAD);  // j >= ncols
  CHECK(ha_hh_step(dummy, 0, 10, 4, 0, 0, -1, 4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
        BAD);  // coff < 0
  CHECK(ha_threefry_fill(dummy, 0, 0, 0, 0, 1, 32, 0, 0.0, 1.0, nullptr) == OK);
  CHECK(ha_threefry_fill(dummy, 0, 4, 0, 0, 1, 16, 0, 0.0, 1.0, nullptr) == BAD);
  CHECK(ha_knn_rescore(nullptr, 4, nullptr, 4, 10, 5, 4, nullptr, 0, 33, 8, nullptr, nullptr, nullptr) == BAD);  // c > 32
  CHECK(ha_knn_rescore(nullptr, 4, nullptr, 4, 10, 5, 4, nullptr, 0, 16, 17, nullptr, nullptr, nullptr) == BAD);  // k > c
  CHECK(ha_knn_rescore(nullptr, 2, nullptr, 4, 10, 5, 4, nullptr, 0, 16, 8, nullptr, nullptr, nullptr) == BAD);  // ldq < f
  CHECK(ha_knn_rescore(nullptr, 4, nullptr, 4, 10, 0, 4, nullptr, 0, 16, 8, nullptr, nullptr, nullptr) == OK);   // nq = 0
  // k-medians: the label order's workspace, the digit table's capacity, the wrappers' rejections
  const int64_t cap = (int64_t)256 << 20;
  for (int64_t n : sizes)
    for (int k : {1, 7, 128, 4096}) {
      const int64_t w = ha_km_label_order_workspace(n, k), c = ha_km_label_order_cstart(n, k);
      CHECK(w >= n + 3 * (int64_t)k + 1 && c >= n && c + k + 1 <= w);
      for (int f : {1, 3, 64, 65}) {
        const int64_t b = ha_med_table_bytes(k, f, cap);
        CHECK(b == ((int64_t)k * f * 1024 <= cap ? (int64_t)k * f * 1024 : -1));
      }
    }
  CHECK(ha_km_label_order_workspace(10, 0) == -1 && ha_km_label_order_workspace((int64_t)1 << 31, 4) == -1);
  CHECK(ha_med_table_bytes(0, 4, cap) == -1 && ha_med_table_bytes(4, 0, cap) == -1);
  CHECK(ha_med_table_bytes(4096, 65, cap) == -1);  // cap exceeded
  CHECK(ha_l1_point_block() > 0 && ha_med_segment() > 0);
  for (int k : {1, 16, 17, 1000}) CHECK(ha_l1_centroid_tile(k) % 16 == 0);
  int idummy[16] = {0};
  CHECK(ha_km_label_order(nullptr, 4, 2, idummy, nullptr) == BAD);
  CHECK(ha_km_label_order(idummy, 4, 2, nullptr, nullptr) == BAD);
  CHECK(ha_km_label_order(idummy, 4, 0, idummy, nullptr) == UNSUP);
  CHECK(ha_l1_assign(nullptr, 0, 4, 4, 4, dummy, 2, 4, idummy, nullptr, nullptr) == BAD);
  CHECK(ha_l1_assign(dummy, 0, 4, 4, 4, nullptr, 2, 4, idummy, nullptr, nullptr) == BAD);
  CHECK(ha_l1_assign(dummy, 0, 4, 4, 4, dummy, 2, 4, nullptr, nullptr, nullptr) == BAD);
  CHECK(ha_l1_assign(dummy, 0, 4, 4, 4, dummy, 0, 4, idummy, nullptr, nullptr) == BAD);   // k <= 0
  CHECK(ha_l1_assign(dummy, 0, 4, 0, 4, dummy, 2, 4, idummy, nullptr, nullptr) == BAD);   // f <= 0
  CHECK(ha_l1_assign(dummy, 0, 4, 4, 2, dummy, 2, 4, idummy, nullptr, nullptr) == BAD);   // ldx < f
  CHECK(ha_l1_assign(dummy, 2, 4, 4, 4, dummy, 2, 4, idummy, nullptr, nullptr) == BAD);   // dtype
  CHECK(ha_l1_assign(dummy, 0, 0, 4, 4, dummy, 2, 4, idummy, nullptr, nullptr) == OK);    // n = 0
  CHECK(ha_l1_to_label(dummy, 0, 4, 4, 4, dummy, 2, 4, nullptr, dummy, nullptr) == BAD);
  CHECK(ha_l1_to_label(dummy, 0, 4, 4, 4, dummy, -1, 4, idummy, dummy, nullptr) == BAD);  // k <= 0
  CHECK(ha_l1_to_label(dummy, 1, 4, -3, 4, dummy, 2, 4, idummy, dummy, nullptr) == BAD);  // f <= 0
  CHECK(ha_med_minmax(nullptr, 0, 4, 4, 4, idummy, idummy, 2, dummy, nullptr) == BAD);
  CHECK(ha_med_minmax(dummy, 0, 4, 4, 4, idummy, idummy, 0, dummy, nullptr) == BAD);      // k <= 0
  CHECK(ha_med_minmax(dummy, 0, 4, 0, 4, idummy, idummy, 2, dummy, nullptr) == BAD);      // f <= 0
  CHECK(ha_med_setup(0, dummy, dummy, 2, 4, dummy, nullptr, idummy, idummy, nullptr) == BAD);
  CHECK(ha_med_setup(0, dummy, dummy, 0, 4, dummy, dummy, idummy, idummy, nullptr) == BAD);
  CHECK(ha_med_select(dummy, 0, 4, 4, 4, idummy, idummy, 2, dummy, dummy, idummy, 0, nullptr, 8192, nullptr) == BAD);
  CHECK(ha_med_select(dummy, 0, 4, 4, 4, idummy, idummy, 2, dummy, dummy, idummy, 4, dummy, 8192, nullptr) == BAD);
  CHECK(ha_med_select(dummy, 0, 4, 4, 4, idummy, idummy, 2, dummy, dummy, idummy, 0, dummy, 8191, nullptr) ==
        UNSUP);  // table smaller than k f 1 KB
  CHECK(ha_med_pick(0, 2, 4, 0, dummy, 8191, dummy, dummy, idummy, nullptr) == UNSUP);
  CHECK(ha_med_pick(0, 2, 4, 0, nullptr, 8192, dummy, dummy, idummy, nullptr) == BAD);
  CHECK(ha_med_pick(1, 2, 0, 0, dummy, 8192, dummy, dummy, idummy, nullptr) == BAD);      // f <= 0
  CHECK(ha_med_fixup(dummy, 0, 4, 4, 4, idummy, idummy, 2, dummy, dummy, nullptr, nullptr) == BAD);
  CHECK(ha_med_fixup(dummy, 0, 4, 4, 4, idummy, idummy, -2, dummy, dummy, dummy, nullptr) == BAD);
  CHECK(ha_med_finish(0, 2, 4, dummy, dummy, dummy, dummy, nullptr, nullptr) == BAD);
  CHECK(ha_med_finish(0, 0, 4, dummy, dummy, dummy, dummy, dummy, nullptr) == BAD);       // k <= 0
  // order statistics: table sizes, pass counts, and what the launchers reject before any device work
  const int maxr = ha_qsel_max_targets();
  CHECK(maxr >= ha_qsel_group() && ha_qsel_group() >= 2);
  CHECK(ha_qsel_passes(0, 0) == 3 && ha_qsel_passes(1, 0) == 6 && ha_qsel_passes(0, 1) == 4 && ha_qsel_passes(1, 1) == 8);
  CHECK(ha_qsel_small_len(0) == 2 * ha_qsel_small_len(1) && ha_qsel_small_len(1) > 0);
  for (int layout : {0, 1})
    for (int64_t slices : {(int64_t)1, (int64_t)7, (int64_t)1000, (int64_t)1 << 20}) {
      const int64_t nb = layout ? 256 : 2048;
      CHECK(ha_qsel_table_elems(layout, slices, 3, 0, INT64_MAX) == slices * (nb + 1));
      CHECK(ha_qsel_table_elems(layout, slices, 3, 2, INT64_MAX) == slices * 3 * (nb + 64));
      CHECK(ha_qsel_table_elems(layout, slices, 3, 1, slices * 3 * (nb + 64) - 1) == -1);  // above the cap
    }
  CHECK(ha_qsel_table_elems(2, 4, 1, 0, cap) == -1 && ha_qsel_table_elems(0, 0, 1, 0, cap) == -1);
  CHECK(ha_qsel_table_elems(0, 4, 0, 0, cap) == -1 && ha_qsel_table_elems(0, 4, maxr + 1, 1, cap) == -1);
  CHECK(ha_qsel_table_elems(1, (int64_t)1 << 31, 1, 0, INT64_MAX) == -1);
  long long ldummy[16] = {0};
  CHECK(ha_qsel_rows_small(dummy, 0, 1, 16, 16, nullptr, 1, dummy, nullptr) == BAD);
  CHECK(ha_qsel_rows_small(dummy, 2, 1, 16, 16, ldummy, 1, dummy, nullptr) == BAD);       // dtype
  CHECK(ha_qsel_rows_small(dummy, 0, 2, 16, 8, ldummy, 1, dummy, nullptr) == BAD);        // ld < len
  CHECK(ha_qsel_rows_small(dummy, 0, 0, 16, 16, ldummy, 1, dummy, nullptr) == OK);        // no rows
  CHECK(ha_qsel_rows_small(dummy, 0, 1, ha_qsel_small_len(0) + 1, 1 << 20, ldummy, 1, dummy, nullptr) == UNSUP);
  CHECK(ha_qsel_rows_small(dummy, 1, 1, 16, 16, ldummy, maxr + 1, dummy, nullptr) == UNSUP);
  CHECK(ha_qsel_rows_pass(dummy, 0, 0, 0, 1, 16, 16, 1, 3, 1, 0, 1, 0, ldummy, idummy, ldummy, 4096, nullptr, nullptr, 0,
                          nullptr) == BAD);  // float32 has 3 passes of 11 bits
  CHECK(ha_qsel_rows_pass(dummy, 0, 0, 0, 1, 16, 16, 1, 1, 9, 0, 9, 0, ldummy, idummy, ldummy, 1 << 20, nullptr, nullptr,
                          0, nullptr) == BAD);  // more targets than a launch takes
  CHECK(ha_qsel_rows_pass(dummy, 0, 0, 0, 1, 16, 16, 1, 1, 2, 0, 2, 1, ldummy, idummy, ldummy, 1 << 20, nullptr, nullptr,
                          0, nullptr) == BAD);  // append without a buffer
  CHECK(ha_qsel_rows_pass(dummy, 0, 0, 1, 1, 16, 16, 1, 1, 2, 0, 2, 0, ldummy, idummy, ldummy, 1 << 20, dummy, ldummy,
                          4, nullptr) == BAD);  // compacted keys exist from pass 2 on
  CHECK(ha_qsel_rows_pass(dummy, 0, 0, 0, 1, 16, 16, 1, 1, 2, 0, 2, 0, nullptr, idummy, ldummy, 1 << 20, nullptr,
                          nullptr, 0, nullptr) == BAD);  // pass 1 without prefixes
  CHECK(ha_qsel_rows_pass(dummy, 0, 0, 0, 0, 16, 16, 1, 0, 1, 0, 1, 0, nullptr, nullptr, ldummy, 16, nullptr, nullptr, 0,
                          nullptr) == OK);  // no slices
  CHECK(ha_qsel_rows_pass(dummy, 0, 0, 0, 1, 16, 16, 1, 0, 1, 0, 1, 0, nullptr, nullptr, ldummy, 2048, nullptr, nullptr,
                          0, nullptr) == UNSUP);  // table smaller than [1][2048] + 1
  CHECK(ha_qsel_rows_pass(dummy, 0, 0, 0, 1, (int64_t)1 << 40, (int64_t)1 << 40, 1, 0, 1, 0, 1, 0, nullptr, nullptr,
                          ldummy, 4096, nullptr, nullptr, 0, nullptr) == UNSUP);  // 2^40 elements in one chunk
  CHECK(ha_qsel_cols_pass(dummy, 0, 4, 4, 2, 1, 0, 1, 0, 1, 0, nullptr, nullptr, ldummy, 4096, nullptr, nullptr, 0,
                          nullptr) == BAD);  // ld < ncols
  CHECK(ha_qsel_cols_pass(dummy, 0, 4, 4, 4, 1, 4, 1, 0, 1, 0, ldummy, idummy, ldummy, 4096, nullptr, nullptr, 0,
                          nullptr) == BAD);  // float32 has 4 passes of 8 bits
  CHECK(ha_qsel_cols_pass(dummy, 1, 4, 4, 4, 1, 0, 1, 0, 1, 0, nullptr, nullptr, ldummy, 4 * 257 - 1, nullptr, nullptr, 0,
                          nullptr) == UNSUP);  // table smaller than [4][256] + 4
  CHECK(ha_qsel_cols_pass(dummy, 1, 0, 4, 4, 1, 0, 1, 0, 1, 0, nullptr, nullptr, ldummy, 16, nullptr, nullptr, 0,
                          nullptr) == OK);  // no rows
  CHECK(ha_qsel_pick(0, 0, 1, 1, 0, nullptr, ldummy, 4096, ldummy, ldummy, ldummy, idummy, ldummy, ldummy, ldummy,
                     nullptr) == BAD);
  CHECK(ha_qsel_pick(0, 1, 1, 1, 0, ldummy, ldummy, 256, ldummy, ldummy, ldummy, idummy, ldummy, ldummy, ldummy,
                     nullptr) == UNSUP);  // table smaller than [1][256] + 1
  CHECK(ha_qsel_pick(1, 1, 1, 1, 8, ldummy, ldummy, 4096, ldummy, ldummy, ldummy, idummy, ldummy, ldummy, ldummy,
                     nullptr) == BAD);  // float64 has 8 passes of 8 bits
  CHECK(ha_qsel_finish(0, 4, 1, ldummy, ldummy, nullptr, nullptr) == BAD);
  CHECK(ha_qsel_finish(0, 4, maxr + 1, ldummy, ldummy, dummy, nullptr) == BAD);
  CHECK(ha_qsel_finish(1, 0, 1, ldummy, ldummy, dummy, nullptr) == OK);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("asan host check ok\n");
  return 0;
}
