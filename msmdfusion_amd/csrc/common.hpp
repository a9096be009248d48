// common.hpp -- shared helpers of libmsmd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "../../include/msmd_hip.h"

#define MSMD_EXPORT extern "C" __attribute__((visibility("default")))

namespace msmd {

constexpr int kWave = 64;  // CDNA wavefront
constexpr int kWgradSplitChunk = 2048;  // pairs per workgroup of the split wgrad kernel

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Launch errors are tracked per call, not through the runtime's sticky "last
// error": PyTorch's allocator leaves hipErrorNotReady (event polling) behind,
// which a bare hipGetLastError() after our launches would misreport.
inline thread_local int g_launch_err = 0;   // first failing hipError_t of this call
inline thread_local int g_last_detail = 0;  // kept for msmd_last_launch_error()
#define MSMD_LAUNCH(kernel, grid, block, smem, stream, ...)                       \
  do {                                                                            \
    (void)hipGetLastError();                                                      \
    hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);           \
    hipError_t e_ = hipGetLastError();                                            \
    if (e_ != hipSuccess && !::msmd::g_launch_err) ::msmd::g_launch_err = (int)e_; \
  } while (0)

// XCD-aware work assignment of the wgrad kernels.  The dispatcher places block b
// on XCD b % 8 (observed, MI355X_MICROARCH.md); each XCD has its own 4 MiB L2.
// The (chunk, offset k, slab) workgroups of one chunk gather the same ~2k feature
// rows: give every XCD whole chunks (chunk % 8 == xcd) and walk (k, slab) for a
// chunk in consecutive blocks of that XCD, so the rows are fetched from HBM once
// per chunk instead of once per (k, slab).  Bijective over
// [0, wgrad_grid(nchunks, kvol, slabs)).
inline int wgrad_grid(int nchunks, int kvol, int slabs) {
  return ((nchunks + 7) / 8) * 8 * kvol * slabs;
}
__device__ __forceinline__ bool wgrad_work(int nchunks, int kvol, int slabs, int& chunk, int& k,
                                           int& slab) {
  const int b = blockIdx.x, xcd = b & 7, j = b >> 3;
  const int per = kvol * slabs;
  const int cg = j / per, r = j - cg * per;
  chunk = cg * 8 + xcd;
  k = r / slabs;
  slab = r - k * slabs;
  return chunk < nchunks;
}

inline int launch_status() {
  int e = g_launch_err;
  g_launch_err = 0;
  if (e) g_last_detail = e;
  return e ? MSMD_ERR_LAUNCH : MSMD_OK;
}

// Dynamic LDS beyond 64 KB is an opt-in per kernel AND per device.  `granted` (one static
// array per call site = per kernel instantiation) remembers the size opted into on each
// device; a mutex orders the threads that call into the library (step thread, index
// prefetcher), and a refused opt-in is reported here instead of as a launch error later.
constexpr int kMaxDevices = 16;
struct LdsGrant {
  size_t bytes[kMaxDevices] = {0};
};
inline int optin_dynamic_lds(const void* kernel, size_t bytes, LdsGrant& g) {
  static std::mutex mu;
  if (bytes > 160 * 1024) return MSMD_ERR_UNSUPPORTED;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return MSMD_ERR_LAUNCH;
  std::lock_guard<std::mutex> lock(mu);
  if (bytes <= g.bytes[dev] || bytes <= 64 * 1024) return MSMD_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
      hipSuccess) {
    (void)hipGetLastError();
    return MSMD_ERR_UNSUPPORTED;
  }
  g.bytes[dev] = bytes;
  return MSMD_OK;
}

// Bump allocator over the caller's workspace (256-B aligned slices).
struct Arena {
  char* base;
  size_t off = 0, cap;
  Arena(void* p, size_t bytes) : base((char*)p), cap(bytes) {}
  template <typename T>
  T* take(size_t n) {
    size_t o = off;
    off = align_up(off + n * sizeof(T));
    return (T*)(base + o);
  }
  bool ok() const { return off <= cap && ((uintptr_t)base & 255) == 0; }
};
// Same arithmetic without memory, for the *_workspace_bytes() queries.
struct ArenaSize {
  size_t off = 0;
  template <typename T>
  T* take(size_t n) { off = align_up(off + n * sizeof(T)); return nullptr; }
};

inline int next_pow2_bits(long v) {  // smallest b with (1<<b) >= v
  int b = 0;
  while ((1L << b) < v) ++b;
  return b;
}

// ---- 32-bit key -> slot hash (multiplicative, table size 2^bits) ----------
// (A locality-preserving "8 consecutive x share one 64-byte bucket" variant was
// measured and rejected: with linear probing the occupied buckets of dense
// scan lines overflow into each other -- voxelization of the 1.1 M-point
// stress case went from 0.56 ms to 2.7 ms, the SubM lookup gained only 6 %.)
__device__ __forceinline__ uint32_t hash_slot(uint32_t key, int bits) {
  return (key * 0x9E3779B1u) >> (32 - bits);
}
constexpr uint64_t kEmptySlot = 0xFFFFFFFFFFFFFFFFull;

// Insert (key -> val) keeping, for equal keys, min(val) (KeepMax=false) or
// max(val).  Slot = key<<32 | val in one 64-bit word: one CAS claims it, one
// atomicMin/Max merges duplicates.  Returns the slot index.
template <bool KeepMax>
__device__ __forceinline__ uint32_t hash_insert(unsigned long long* table, int bits,
                                                uint32_t key, uint32_t val) {
  const uint32_t mask = (1u << bits) - 1;
  uint32_t h = hash_slot(key, bits);
  const unsigned long long packed = ((unsigned long long)key << 32) | val;
  while (true) {
    unsigned long long cur = table[h];
    if (cur == kEmptySlot) {
      cur = atomicCAS(&table[h], (unsigned long long)kEmptySlot, packed);
      if (cur == kEmptySlot) return h;
    }
    if ((uint32_t)(cur >> 32) == key) {
      if (KeepMax) atomicMax(&table[h], packed); else atomicMin(&table[h], packed);
      return h;
    }
    h = (h + 1) & mask;
  }
}

// Lookup: value stored for key, or -1.
__device__ __forceinline__ int hash_find(const unsigned long long* __restrict__ table,
                                         int bits, uint32_t key) {
  const uint32_t mask = (1u << bits) - 1;
  uint32_t h = hash_slot(key, bits);
  while (true) {
    unsigned long long cur = table[h];
    if (cur == kEmptySlot) return -1;
    if ((uint32_t)(cur >> 32) == key) return (int)(uint32_t)cur;
    h = (h + 1) & mask;
  }
}

// ---- wave / block reductions ---------------------------------------------
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// exclusive prefix of v over the 64 lanes of a wave
__device__ __forceinline__ int wave_excl_scan(int v, int lane) {
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  return x - v;
}

// Exclusive scan of one int per thread across a block of BLOCK threads.
// smem needs BLOCK/64 ints.  Returns the exclusive prefix; *total = block sum.
template <int BLOCK>
__device__ __forceinline__ int block_excl_scan(int v, int* smem, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int ex = wave_excl_scan(v, lane);
  if (lane == 63) smem[w] = ex + v;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < BLOCK / 64; ++i) {
    int s = smem[i];
    if (i < w) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return ex + base;
}

}  // namespace msmd
