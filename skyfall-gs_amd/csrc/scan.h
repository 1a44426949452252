// scan.h -- the TOP level of a device-wide exclusive scan, once: every caller (compact, densify, mesh's adjacency, pointcloud,
// tsdf, knn) first leaves one sum per workgroup with a kernel of its own, then ONE workgroup of SCAN_TOP_THREADS threads walks
// those sums here, and a third kernel of the caller's adds each workgroup's prefix to its local ranks. No kernel waits for
// another workgroup. The per-workgroup kernels stay with their callers: they differ in what a row's value is.
#pragma once
#include "sfgs_internal.h"

namespace sfgs {

constexpr int SCAN_TOP_THREADS = 1024;

// sums[i * stride], i < NB: sum -> carry + the exclusive prefix, SCAN_TOP_THREADS per round; returns carry + the total. Called by
// every thread of a SCAN_TOP_THREADS workgroup; NB is uniform, so every thread reaches every barrier. smem: SCAN_TOP_THREADS / 64
// + 1 words. A round's sums are taken as 32-bit words and so is its total (the callers' chunk sizes keep it below 2^32); the
// carry is 64 bits wide, and a 32-bit T keeps its low word: (unsigned)(carry + ex) == (unsigned)carry + ex.
template <typename T>
__device__ __forceinline__ unsigned long long scan_sums_excl(T* sums, long long NB, long long stride, unsigned long long carry,
                                                             unsigned* smem) {
  for (long long b0 = 0; b0 < NB; b0 += SCAN_TOP_THREADS) {
    const long long i = b0 + threadIdx.x;
    const unsigned v = i < NB ? (unsigned)sums[i * stride] : 0u;
    unsigned total;
    const unsigned ex = block_excl_scan_u32<SCAN_TOP_THREADS>(v, &total, smem);
    if (i < NB) sums[i * stride] = (T)(carry + ex);
    carry += total;
  }
  return carry;
}

// sums: [NB][cats], category k scanned on its own. carry_in (null: zeros) and totals (null: not wanted) hold a word per category
// and may be the SAME words (pointcloud's running row count): every thread reads its starting carry before the first barrier,
// thread 0 writes the total after the last. Hence no __restrict__ on that pair.
// static: every file that launches it gets a copy in its own code object. With external linkage the files share one host handle,
// the first file's code object serves them all, and sfgs_tsdf_extract -- count and emit from tsdf.hip, the scan from
// pointcloud.hip -- measured 15 us (1.5 %) longer per call with equal kernel times (profiles/r26_scan_rows_ab.txt).
template <typename T>
static __global__ void __launch_bounds__(SCAN_TOP_THREADS)
scan_sums_kernel(T* __restrict__ sums, long long NB, int cats, const unsigned long long* carry_in, unsigned long long* totals) {
  __shared__ unsigned smem[SCAN_TOP_THREADS / 64 + 1];
  for (int k = 0; k < cats; ++k) {
    const unsigned long long total = scan_sums_excl(sums + k, NB, (long long)cats, carry_in ? carry_in[k] : 0ull, smem);
    if (totals && threadIdx.x == 0) totals[k] = total;
  }
}

}  // namespace sfgs
