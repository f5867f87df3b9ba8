// The fp64 MFMA staging ring of gemm_f64.hip, cdist_f64.hip, kmeans_f64.hip and knn_f64.hip: how
// two operands of a 128 x 128 tile of v_mfma_f64_16x16x4_f64 work get from global memory into LDS.
// Here: the description of the pipeline, its geometry, the per-lane source descriptor and the
// row-norm pre-pass of the three distance kernels; the DMA and the counted waits are in common.h.
// The stage / zero_tail / ready lambdas and the driving loop that use them are still written out
// in each kernel, next to its fragment reads, accumulator map and epilogue: moved into one struct
// here they compiled to other code in every kernel (other instruction order throughout, 2 - 4
// more VGPRs in cdist_f64_mm, 16 bytes of scratch in kn64_topk<16>;
// profiles/f64_ring_refactor.md), and these kernels sit at 213 - 256 VGPRs with two workgroups
// per CU to keep.
//
// The pipeline:
//   * a stage is 8 k of both operands, 128 rows each: 8 KB per operand, 16 KB per stage, moved by
//     asm LDS-DMA (ha_dma16, 1 KB per wave-instruction): 8 pieces per operand, each of the 4 waves
//     issues 2 of the first operand and 2 of the second (F64_DPS = 4 per wave per stage);
//   * the stages live in a ring of NBUF slots (4, or 3 where the kernel needs the LDS), NBUF - 1 in
//     flight. A stage is waited for with a COUNTED vmcnt - the DMAs of the stages issued after it
//     stay outstanding - and one raw s_barrier (ha_wait_barrier); never vmcnt(0) in the steady
//     state. The barrier that publishes stage t also says that every wave has read stage t - 1,
//     whose slot stage t + NBUF - 1 is then issued into;
//   * images. A k-contiguous operand ([rows][K]) is imaged [k/2][row][2]: a 16-byte DMA lane is two
//     consecutive k of one row, piece q = k-pair q / 2 of rows 64 (q % 2) + lane. A lane of the
//     f64 fragment map (row lane & 15, k-slot lane >> 4) reads its row's pair kk with ONE
//     ds_read_b128 and feeds both MFMA k-steps of the stage (k-slot kk of step s holds k = 2 kk + s,
//     for both operands alike); 16 lanes read 256 contiguous bytes, conflict-free. A row-contiguous
//     operand ([K][rows], gemm_f64.hip only) is imaged [k][row]: piece q = k-row q, a lane takes
//     rows 2 lane, 2 lane + 1. Either way piece q lands at byte q KB of the operand's image;
//   * out-of-range rows are clamped at the load (the kernels mask them at the store);
//   * K need be no multiple of 8 and may be smaller than the ring: the loop's guarded steps cover
//     fewer stages than slots, down to K = 1. The last stage of such a K (the tail) is loaded with
//     its k clamped into the operand and the entries at k >= K are zeroed in LDS after they land,
//     each wave zeroing the pieces it loaded itself (behind a vmcnt(0), before the stage's barrier);
//   * K may be odd. The 16-byte load of a k-contiguous row's last pair then also takes the 8 bytes
//     behind k = K - 1 and zeroes them like the rest of the tail. In every row but the last these
//     lie inside the (even) leading dimension. In the very last row of a tensor whose storage ends
//     exactly at its last element they are OUT OF THE ALLOCATION: the kernel reads them on purpose.
//     The read cannot fault - the load is 16-byte aligned and its first half is in bounds, so it
//     stays inside that element's page - and its value never reaches a result. The same holds for
//     an odd row count of a row-contiguous operand (the last k-row's last pair). A memory checker
//     that tracks allocation bounds will report it.
// Requirements on every operand: 16-byte aligned, even leading dimension (made so by the callers of
// the kernels, never by a copy in them).
#pragma once
#include "common.h"

namespace {

typedef double doublex2 __attribute__((ext_vector_type(2)));
typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int F64_T = 128;                // tile rows of either operand
constexpr int F64_K = 8;                  // k per stage
constexpr int F64_OP = F64_T * F64_K * 8; // bytes per operand per stage
constexpr int F64_STG = 2 * F64_OP;       // bytes per stage
constexpr int F64_DPS = 4;                // DMA instructions per wave per stage (2 per operand)

// One operand's staging for this lane. KC (k-contiguous, [rows][K] with leading dimension ld):
// piece q = k-pair q / 2 of the stage, rows 64 (q % 2) + lane. Else row-contiguous ([K][rows]):
// piece q = k-row q, rows 2 lane, 2 lane + 1. Out-of-range rows are clamped.
template <bool KC = true>
struct F64Src {
  const double* p0;  // KC: row lane of the tile; else rows 2 lane .. + 1 at k = 0
  const double* p1;  // KC: row 64 + lane
  int64_t ld;
  __device__ __forceinline__ void init(const double* P, int64_t ld_, int64_t rows, int64_t r0, int lane) {
    ld = ld_;
    if (KC) {
      const int64_t a = r0 + lane, b = r0 + 64 + lane;
      p0 = P + (a < rows ? a : rows - 1) * ld;
      p1 = P + (b < rows ? b : rows - 1) * ld;
    } else {
      const int64_t c = r0 + 2 * lane, last = (rows - 1) & ~(int64_t)1;
      p0 = p1 = P + (c < last ? c : last);
    }
  }
  // source of piece q of the stage at k0 (whole stage in range)
  __device__ __forceinline__ const double* src(int64_t k0, int q) const {
    return KC ? ((q & 1) ? p1 : p0) + k0 + 2 * (q >> 1) : p0 + (k0 + q) * ld;
  }
  // the same with k clamped into the operand (the tail stage)
  __device__ __forceinline__ const double* src_clamped(int64_t k0, int q, int64_t K) const {
    if (KC) {
      const int64_t k = k0 + 2 * (q >> 1), last = (K - 1) & ~(int64_t)1;
      return ((q & 1) ? p1 : p0) + (k < last ? k : last);
    }
    const int64_t k = k0 + q;
    return p0 + (k < K ? k : K - 1) * ld;
  }
  // first k of piece q's two values (KC: k, k + 1; else both values at this k)
  __device__ __forceinline__ int64_t kfirst(int64_t k0, int q) const { return KC ? k0 + 2 * (q >> 1) : k0 + q; }
};

// out[i] = |row i|^2 for the rows of A (i < na) then of B (i - na < nb; nb = 0: A only). 16 lanes
// per row, lane l sums features l, l + 16, ... in order, then a fixed xor tree: bit-identical for a
// row wherever it sits.
__global__ __launch_bounds__(256) void f64_row_norms(const double* __restrict__ A, int64_t na, int64_t lda,
                                                     const double* __restrict__ B, int64_t nb, int64_t ldb,
                                                     int64_t f, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  if (i >= na + nb) return;  // whole 16-lane groups leave together
  const double* row = i < na ? A + i * lda : B + (i - na) * ldb;
  double s = 0.0;
  for (int64_t k = l; k < f; k += 16) s = fma(row[k], row[k], s);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
  if (l == 0) out[i] = s;
}

}  // namespace
