// compact.hip -- row compaction of MANY tensors by one keep-mask in one pass.
// Reference: GaussianModel.prune_points / _prune_optimizer (scene/gaussian_model.py:563-603): every parameter, both
// Adam moments of every parameter and five per-Gaussian statistics tensors are filtered with `tensor[mask]` -- 26
// boolean-index operations, each of which runs its own mask -> index conversion (nonzero) and waits for the host to
// learn the output size. Here: ONE prefix scan of the mask (one host read-back: the kept-row count, needed to size the
// outputs) and ONE multi-tensor gather launch. Pure data movement: bit-exact by construction.
#include "sfgs_internal.h"
#include "row_table.h"
#include "scan.h"

namespace sfgs {

constexpr int CP_MAX_TENSORS = 48;

// CompactScratch / cp_blocks / cp_scratch_bytes / cp_view: sfgs_internal.h (mesh.hip reads a plan's ranks too)

__global__ void __launch_bounds__(CP_NT)
compact_count_kernel(const unsigned char* __restrict__ keep, long long N, unsigned* __restrict__ block_sum) {
  __shared__ unsigned smem[CP_NT / 64 + 1];
  const long long base = (long long)blockIdx.x * CP_CHUNK + (long long)threadIdx.x * CP_ROWS_PER_THREAD;
  unsigned c = 0;
  unsigned char kv[CP_ROWS_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k) kv[k] = keep[min(base + k, N - 1)];   // loads first (see compact_gather)
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k) c += (base + k < N && kv[k]) ? 1u : 0u;
  unsigned total;
  block_excl_scan_u32<CP_NT>(c, &total, smem);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(CP_NT)
compact_index_kernel(const unsigned char* __restrict__ keep, long long N, const unsigned* __restrict__ block_sum,
                     unsigned* __restrict__ dst_index) {
  __shared__ unsigned smem[CP_NT / 64 + 1];
  const long long base = (long long)blockIdx.x * CP_CHUNK + (long long)threadIdx.x * CP_ROWS_PER_THREAD;
  unsigned flags = 0, c = 0;
  unsigned char kv[CP_ROWS_PER_THREAD];
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k) kv[k] = keep[min(base + k, N - 1)];
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k)
    if (base + k < N && kv[k]) { flags |= 1u << k; ++c; }
  unsigned total;
  unsigned pos = block_sum[blockIdx.x] + block_excl_scan_u32<CP_NT>(c, &total, smem);
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k)
    if (base + k < N) { dst_index[base + k] = pos; pos += (flags >> k) & 1u; }
}

using CompactTable = RowTable<CP_MAX_TENSORS>;

template <typename U>
__global__ void __launch_bounds__(RT_NT)
compact_gather_kernel(const CompactTable tab, const unsigned char* __restrict__ keep,
                      const unsigned* __restrict__ dst_index, long long N) {
  // three phases so that every load of the thread is in flight before the first use: rows and keep flags, then
  // destination rows and source words (unconditional, from clamped indices), then the predicated stores. (One loop with
  // `if (keep[row]) dst[..dst_index[row]..] = src[w]` serialises three dependent round trips per word.)
  long long rowv[RT_WORDS_PER_THREAD];
  unsigned colv[RT_WORDS_PER_THREAD];
  unsigned char kp[RT_WORDS_PER_THREAD];
  const RowWalk rw = row_table_walk(tab, N, keep, rowv, colv, kp);
  const U* __restrict__ src = (const U*)rw.src;
  U* __restrict__ dst = (U*)rw.dst;
  U val[RT_WORDS_PER_THREAD];
  unsigned di[RT_WORDS_PER_THREAD];
#pragma unroll
  for (int k = 0; k < RT_WORDS_PER_THREAD; ++k) {
    const long long w = min(rw.base + (long long)(threadIdx.x + k * RT_NT), rw.words - 1);
    val[k] = src[w];
    di[k] = dst_index[rowv[k]];
  }
#pragma unroll
  for (int k = 0; k < RT_WORDS_PER_THREAD; ++k) {
    const long long w = rw.base + (long long)(threadIdx.x + k * RT_NT);
    if (w < rw.words && kp[k]) dst[(long long)di[k] * rw.ru + colv[k]] = val[k];
  }
}

}  // namespace sfgs

using namespace sfgs;

extern "C" size_t sfgs_compact_scratch_bytes(int64_t N) { return N < 0 ? 0 : cp_scratch_bytes(N); }

extern "C" int sfgs_compact_plan(const unsigned char* keep, int64_t N, void* scratch, size_t scratch_sz,
                                 int64_t* kept_out, void* stream_) {
  SFGS_REQUIRE(N >= 0 && N < (1ll << 32), SFGS_E_ARG, "row count out of range");
  SFGS_REQUIRE(scratch && scratch_sz >= cp_scratch_bytes(N), SFGS_E_CAPACITY, "compact scratch too small");
  hipStream_t stream = (hipStream_t)stream_;
  const CompactScratch s = cp_view(scratch, N);
  if (N == 0) {
    SFGS_CHECK_HIP(hipMemsetAsync(s.total, 0, 8, stream));
  } else {
    SFGS_REQUIRE(keep, SFGS_E_ARG, "NULL mask");
    const long long NB = cp_blocks(N);
    { ProfScope ps_(KID_COMPACT_SCAN, stream);
      hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)NB), dim3(CP_NT), 0, stream, keep, (long long)N, s.block_sum);
      hipLaunchKernelGGL(scan_sums_kernel<unsigned>, dim3(1), dim3(SCAN_TOP_THREADS), 0, stream, s.block_sum, NB, 1,
                         (const unsigned long long*)nullptr, s.total);
      hipLaunchKernelGGL(compact_index_kernel, dim3((unsigned)NB), dim3(CP_NT), 0, stream, keep, (long long)N,
                         s.block_sum, s.dst_index); }
    SFGS_POST_LAUNCH("compact_scan", stream, 0);
  }
  if (kept_out) {  // the one host synchronisation of a prune: the caller sizes its outputs with this
    unsigned long long h = 0;
    SFGS_CHECK_HIP(hipMemcpyAsync(&h, s.total, 8, hipMemcpyDeviceToHost, stream));
    SFGS_CHECK_HIP(hipStreamSynchronize(stream));
    *kept_out = (int64_t)h;
  }
  return SFGS_OK;
}

extern "C" int sfgs_compact_rows(const unsigned char* keep, int64_t N, const void* scratch,
                                 const SfgsCompactTensor* tensors, int32_t count, void* stream_) {
  SFGS_REQUIRE(N >= 0 && N < (1ll << 32) && count >= 0, SFGS_E_ARG, "bad row / tensor count");
  if (N == 0 || count == 0) return SFGS_OK;
  SFGS_REQUIRE(keep && scratch && tensors, SFGS_E_ARG, "NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  const CompactScratch s = cp_view(const_cast<void*>(scratch), N);
  bool words_ok = true;  // 4-byte units when every tensor allows it, bytes otherwise
  for (int i = 0; i < count; ++i) {
    SFGS_REQUIRE(tensors[i].row_bytes >= 0 && tensors[i].row_bytes < (1ll << 22), SFGS_E_ARG, "tensor %d: bad row size", i);
    if (tensors[i].row_bytes == 0) continue;
    SFGS_REQUIRE(tensors[i].src && tensors[i].dst, SFGS_E_ARG, "tensor %d: NULL pointer", i);
    if ((tensors[i].row_bytes & 3) || (((uintptr_t)tensors[i].src | (uintptr_t)tensors[i].dst) & 3)) words_ok = false;
  }
  const int unit = words_ok ? 4 : 1;
  int i = 0;
  while (i < count) {
    CompactTable tab;
    uint64_t blocks;
    if (const int rc = row_table_pack(tensors, count, i, N, unit, &tab, &blocks, &i)) return rc;
    if (!blocks) break;
    { ProfScope ps_(KID_COMPACT_GATHER, stream);
      if (words_ok) hipLaunchKernelGGL(compact_gather_kernel<uint32_t>, dim3((unsigned)blocks), dim3(RT_NT), 0, stream, tab, keep, s.dst_index, (long long)N);
      else hipLaunchKernelGGL(compact_gather_kernel<unsigned char>, dim3((unsigned)blocks), dim3(RT_NT), 0, stream, tab, keep, s.dst_index, (long long)N); }
    SFGS_POST_LAUNCH("compact_gather", stream, 0);
  }
  return SFGS_OK;
}
