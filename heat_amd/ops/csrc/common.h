// Shared helpers for the heat_amd CDNA4 (gfx950) kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

#define HA_EXPORT extern "C" __attribute__((visibility("default")))

// status codes returned to Python
enum { HA_OK = 0, HA_BAD_ARG = 1, HA_UNSUPPORTED = 2, HA_LAUNCH = 3 };

static inline int ha_launch_status() { return hipGetLastError() == hipSuccess ? HA_OK : HA_LAUNCH; }

__device__ __forceinline__ float ha_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double ha_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Tile order for a 1-D grid on the 8 XCDs (workgroup i runs on XCD i % 8): each XCD gets a
// contiguous run of tiles. 32-bit: the hosts cap such grids at 2^31 - 1 tiles (64-bit divisions
// are long SALU sequences).
__device__ __forceinline__ unsigned ha_xcd_remap(unsigned orig, unsigned nwg) {
  const unsigned q = nwg / 8, r = nwg % 8, xcd = orig % 8, loc = orig / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// LDS-DMA of 16 bytes per lane (global_load_lds_dwordx4; LDS address = lds + 16 lane) issued
// through inline asm: for the builtin the compiler's wait-count pass cannot tell which LDS bytes
// the transfer writes and puts s_waitcnt vmcnt(0) before the next LDS read - i.e. it waits for
// the prefetched stages too. The asm form is invisible to that pass (its own vmcnt waits only
// become more conservative); the kernels wait for their transfers with the counted
// ha_wait_barrier<N>() / ha_vm_wait<N>().
// M0 (the LDS address of the transfer) is saved and restored around it: the compiler treats M0 as
// reserved and would not see a clobber.
// The LDS address is wave-uniform; readfirstlane pins it to an SGPR (inside a lane-divergent
// branch the compiler may otherwise hand the "s" operand a VGPR).
__device__ __forceinline__ void ha_dma16(const void* g, unsigned lds) {
  unsigned saved;
  const unsigned base = __builtin_amdgcn_readfirstlane(lds);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(saved)
               : "v"(g), "s"(base)
               : "memory");
}

// at most N of this wave's vector-memory ops outstanding (its DMA of the stage about to be read
// has landed), LDS ops retired, then the workgroup barrier. Any N < 64: the count is an assembler
// immediate (an earlier form with one asm string per count fell back to vmcnt(0) for every count
// it did not list). sched_barrier(0) on both sides: register-only MFMAs would otherwise migrate
// across the asm statement, which only orders memory operations.
template <int N>
__device__ __forceinline__ void ha_wait_barrier() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"i"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// the counted wait alone
template <int N>
__device__ __forceinline__ void ha_vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

// Inter-workgroup hand-off inside one launch without a per-block release fence (the
// "write-through stores + counter" form of the CDNA4 visibility rules): every handed-off word is
// stored sc1 (relaxed agent-scope atomic store on a GLOBAL pointer), every storing wave drains
// (s_waitcnt vmcnt(0)) before the workgroup barrier, one lane then takes a ticket with an
// agent-scope atomic add; the workgroup whose add came last does ONE agent acquire (L1
// invalidate) and reads. A release fence per block (buffer_wbl2) serialises per CU: ~9 us per
// block at 8 blocks per CU, measured as +70 us on a 0.64 ms moments pass with 2048 blocks.
typedef __attribute__((address_space(1))) unsigned long long ha_gu64;
typedef __attribute__((address_space(1))) unsigned ha_gu32;

__device__ __forceinline__ void ha_store_wt(double* p, double v) {
  __hip_atomic_store((ha_gu64*)(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// The ticket of that hand-off (moments.hip, moments4.hip). This block's partials are stored
// write-through (ha_store_wt) by the threads that own them; each of those waves drained them
// (s_waitcnt vmcnt(0)) before the barrier here. Lane 0 takes a ticket on the per-output arrival
// counter (agent-scope atomic, no release fence); true in every thread of the block that arrived
// last, after ONE agent acquire, which also resets the counter for the next launch on this
// workspace.
__device__ __forceinline__ bool mom_last_arrival(unsigned* __restrict__ cnt, unsigned expected) {
  __shared__ bool last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add((ha_gu32*)(cnt), 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    const bool l = t == expected - 1;
    if (l) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store((ha_gu32*)(cnt), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    last = l;
  }
  __syncthreads();
  return last;
}
