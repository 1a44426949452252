// raster_binning.hip -- second stage of the forward's plan (map of the forward: raster_fwd.hip): the second pass of the
// two-pass coarse binning (bin_count -> bin_rank -> bin_scatter: the pair list preprocess wrote, sorted by coarse bin) and
// the plan's two single-workgroup scans (counters for the host, published straight into pinned host memory; list-slot
// bases of the bins), which ride in the scatter launch or run as plan_scan. Also the joint render's export and merge of a
// plan (sfgs_raster_plan_export / _merge), which read and rebuild exactly these bins.
#include <algorithm>

#include "sfgs_internal.h"

namespace sfgs {

// ------------------------------------------------------------------------------------------------
// K1s: second pass of the two-pass binning = ONE RADIX PASS over the (coarse bin, item) pairs with the coarse bin as the
// digit, in the classic three steps -- no device atomics at all:
//   bin_count_kernel    one workgroup per SCATTER_BLOCKS consecutive preprocess workgroups (~11 000 pairs on the headline
//                       scene) counts its pairs per coarse bin in LDS (items, tile hits) and writes its row of the
//                       [workgroup][bin] count matrices;
//   bin_rank_kernel     column scan: for every bin the first slab rank of every workgroup's run (behind the items the big
//                       splats appended directly, with atomics, while preprocess ran), and the bin's totals into its
//                       64-bit counter (items | hits, the format of the direct path);
//   bin_scatter_kernel  the same workgroups again: counting-sort their pairs by bin (LDS cursors, 16-bit pair indices)
//                       and write them in SORTED order -- consecutive lanes store consecutive items of a bin's run.
// With one returning device atomic per (workgroup, bin) instead (first version of this round: 0.5 M atomics, all
// workgroups hitting the same 2 040 counter lines at the same moment) the reservation alone took 36 of the pass's 73 us
// (profiles/r3_bin_scatter_ablation.txt). The order of a bin's items is irrelevant (its tiles are sorted afterwards).
// (ablation builds of this kernel -- no sorted stores / no sweeps / no counting: profiles/r3_bin_scatter_ablation.txt)
constexpr int SCATTER_NT = 1024, SCATTER_BINS = 4096, SCATTER_IDX = 15360, SCATTER_MLP = 4;
static_assert(SCATTER_BLOCKS * PAIRS_PER_BLOCK <= 65536, "16-bit pair indices");
static_assert(SCATTER_BLOCKS <= 64, "one wave scans the block counts");

// prefix sums of the workgroup's SCATTER_BLOCKS block counts -> s_prefix[0 .. nblk]; returns the total
__device__ __forceinline__ unsigned scatter_prefix(const uint32_t* __restrict__ block_items, int b0, int nblk,
                                                   unsigned* s_prefix) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const unsigned c = tid < nblk ? block_items[b0 + tid] : 0u;
    const unsigned incl = wave_incl_scan_u32(c);
    if (tid < SCATTER_BLOCKS) s_prefix[tid + 1] = incl;
    if (tid == 0) s_prefix[0] = 0u;
  }
  __syncthreads();
  return s_prefix[nblk];
}
// flat pair index -> address: the preprocess workgroup it belongs to by binary search over <= 33 prefix sums
__device__ __forceinline__ const uint4* scatter_pair(const uint4* __restrict__ pairs, const unsigned* s_prefix, int b0,
                                                     int nblk, unsigned i) {
  int lo = 0, hi = nblk;                 // s_prefix[lo] <= i < s_prefix[hi]
#pragma unroll
  for (int it = 0; it < 6; ++it) {       // 2^6 > SCATTER_BLOCKS
    const int mid = (lo + hi) >> 1;
    if (hi - lo > 1) { if (s_prefix[mid] <= i) lo = mid; else hi = mid; }
  }
  return pairs + (size_t)(b0 + lo) * PAIRS_PER_BLOCK + (i - s_prefix[lo]);
}

__global__ void __launch_bounds__(SCATTER_NT)
bin_count_kernel(int NB, int NCB, const uint4* __restrict__ pairs, const uint32_t* __restrict__ block_items,
                 uint32_t* __restrict__ sc_cnt, uint32_t* __restrict__ sc_hits) {
  __shared__ unsigned s_prefix[SCATTER_BLOCKS + 1];
  __shared__ unsigned s_items[SCATTER_BINS], s_hits[SCATTER_BINS];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * SCATTER_BLOCKS, nblk = min(SCATTER_BLOCKS, NB - b0);
  const unsigned total = scatter_prefix(block_items, b0, nblk, s_prefix);
  for (int r0 = 0; r0 < NCB; r0 += SCATTER_BINS) {   // one round up to 4 096 bins (1080p: 2 040, 2160p: 8 160)
    const int nbins = min(SCATTER_BINS, NCB - r0);
    for (int i = tid; i < nbins; i += SCATTER_NT) { s_items[i] = 0u; s_hits[i] = 0u; }
    __syncthreads();
    for (unsigned i0 = tid; i0 < total; i0 += SCATTER_MLP * SCATTER_NT) {   // independent loads in flight per thread
      unsigned w[SCATTER_MLP];
#pragma unroll
      for (int u = 0; u < SCATTER_MLP; ++u)
        w[u] = i0 + u * SCATTER_NT < total ? scatter_pair(pairs, s_prefix, b0, nblk, i0 + u * SCATTER_NT)->w : 0u;
#pragma unroll
      for (int u = 0; u < SCATTER_MLP; ++u) {
        const int cb = (int)(w[u] >> 16) - r0;
        if ((w[u] & 0xffffu) && cb >= 0 && cb < nbins) {
          atomicAdd(&s_items[cb], 1u);
          atomicAdd(&s_hits[cb], (unsigned)__popc(w[u] & 0xffffu));
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < nbins; i += SCATTER_NT) {   // the whole row, zeros included: the matrices are not cleared
      sc_cnt[(size_t)blockIdx.x * NCB + r0 + i] = s_items[i];
      sc_hits[(size_t)blockIdx.x * NCB + r0 + i] = s_hits[i];
    }
    __syncthreads();
  }
}

// 16 bins (columns) per workgroup, 64 row groups: thread (g, c) owns positions [g R, (g + 1) R) of column c's rank order
// (R = 4 with the headline's 245 rows); 128 workgroups at 1080p
constexpr int RANK_COLS = 16, RANK_GROUPS = 64;
// Rank ORDER of the scatter workgroups inside a bin's slab: XCD-major (workgroup w runs on XCD w mod 8), so that the ~31
// workgroups of one XCD own ONE contiguous stretch of every slab and its partial lines are completed inside that XCD's L2
// instead of being written back piecemeal from eight of them. k-th in rank order -> workgroup (matrix row).
// (rank order = workgroup order measured slower: profiles/r3_bin_rank_xcd_major_ab.txt)
__device__ __forceinline__ int rank_row(int k, int NWG) {
  const int q = NWG >> 3, r = NWG & 7;               // XCDs x < r have q + 1 workgroups, the others q
  int x = 0, first = 0;                              // (compares instead of integer divisions)
#pragma unroll
  for (int t = 1; t < 8; ++t) {
    const int st = min(t, r) * (q + 1) + max(t - r, 0) * q;   // rank position of XCD t's first workgroup
    if (k >= st) { x = t; first = st; }
  }
  return (k - first) * 8 + x;
}
__global__ void __launch_bounds__(RANK_COLS * RANK_GROUPS)
bin_rank_kernel(int NWG, int NCB, const uint32_t* __restrict__ sc_cnt, const uint32_t* __restrict__ sc_hits,
                uint32_t* __restrict__ sc_base, uint32_t* __restrict__ coarse_count, unsigned long long* __restrict__ hdr) {
  __shared__ unsigned s_c[RANK_GROUPS][RANK_COLS], s_h[RANK_GROUPS][RANK_COLS];
  __shared__ unsigned s_tot[RANK_COLS], s_first[RANK_COLS];
  const int c = threadIdx.x % RANK_COLS, g = threadIdx.x / RANK_COLS;
  const int bin = min(blockIdx.x * RANK_COLS + c, NCB - 1);      // (lanes beyond the last bin repeat it and write nothing)
  const bool live = blockIdx.x * RANK_COLS + c < NCB;
  const int R = (NWG + RANK_GROUPS - 1) / RANK_GROUPS;
  const int w0 = min(g * R, NWG), w1 = min(w0 + R, NWG);
  unsigned long long* counter = reinterpret_cast<unsigned long long*>(&coarse_count[(size_t)bin * CC_STRIDE]);
  const unsigned long long old = *counter;           // what the big splats appended directly (preprocess / big_walk are done)
  unsigned sc = 0u, sh = 0u;
  for (int w = w0; w < w1; w += 4) {                  // four rows in flight (clamped: no predicated loads)
    unsigned tc[4], th[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t at = (size_t)rank_row(min(w + u, w1 - 1), NWG) * NCB + bin;
      tc[u] = sc_cnt[at]; th[u] = sc_hits[at];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (w + u < w1) { sc += tc[u]; sh += th[u]; }
  }
  s_c[g][c] = sc; s_h[g][c] = sh;
  __syncthreads();                                   // (every row group has read the counter BEFORE the last one rewrites it)
  // The bins' runs in BinsView::csr are EXACTLY sized: this workgroup takes the room of its 16 bins with ONE device atomic
  // on the header's cursor (128 atomics per frame at 1080p) and lays the bins out one after the other. Which workgroup comes
  // first is a race -- it decides where a bin's run lies, never what it holds.
  if (g == 0) {
    unsigned tot = 0u;
    for (int q = 0; q < RANK_GROUPS; ++q) tot += s_c[q][c];
    s_tot[c] = live ? tot : 0u;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned sum = 0u;
#pragma unroll
    for (int k = 0; k < RANK_COLS; ++k) { s_first[k] = sum; sum += s_tot[k]; }
    const unsigned at = (unsigned)atomicAdd(&hdr[HDR_CSR_CURSOR], (unsigned long long)sum);
#pragma unroll
    for (int k = 0; k < RANK_COLS; ++k) s_first[k] += at;
  }
  __syncthreads();
  unsigned run = s_first[c];                         // position in BinsView::csr
  for (int q = 0; q < g; ++q) run += s_c[q][c];
  for (int w = w0; w < w1; w += 4) {
    unsigned tc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) tc[u] = sc_cnt[(size_t)rank_row(min(w + u, w1 - 1), NWG) * NCB + bin];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (w + u < w1) {
        if (live) sc_base[(size_t)rank_row(w + u, NWG) * NCB + bin] = run;
        run += tc[u];
      }
  }
  if (g == RANK_GROUPS - 1 && live) {
    unsigned hits = (unsigned)(old >> 32);
    for (int q = 0; q < RANK_GROUPS; ++q) hits += s_h[q][c];
    // word 0: ALL items of the bin (the directly appended ones + this run), word 1: their tile hits
    *counter = (unsigned long long)((unsigned)old + s_tot[c]) | ((unsigned long long)hits << 32);
    coarse_count[(size_t)bin * CC_STRIDE + 6] = s_first[c];
    coarse_count[(size_t)bin * CC_STRIDE + 7] = s_tot[c];
  }
}

// the plan's two single-workgroup epilogues (defined below: counters for the host; list-slot bases of the bins)
__device__ void plan_scan_role(int role, int NCB, int NB, uint32_t* __restrict__ coarse_count,
                               const uint32_t* __restrict__ block_nvis, const unsigned long long* __restrict__ block_dref,
                               unsigned long long* __restrict__ hdr, const unsigned long long* __restrict__ feedback,
                               const unsigned long long* __restrict__ dup_pool, unsigned long long* __restrict__ host_out,
                               unsigned coarse_capacity);

// plan_roles = 2: the launch's LAST two workgroups run the plan's epilogues (plan_scan_role) next to the scatter
// workgroups instead of a launch of their own behind them -- everything they read is final before this kernel starts (the
// bins' totals come from bin_rank, the per-block statistics from preprocess), and the one thing the scatter may still
// add, the overflow flag of a bin beyond its capacity, role 0 derives from the fullest bin's count itself. (At the END of
// the grid: scatter workgroup w must be workgroup w of the launch, i.e. run on XCD w mod 8 -- rank_row's slab order
// relies on it)
__global__ void __launch_bounds__(SCATTER_NT)
bin_scatter_kernel(int NB, int NCB, const uint4* __restrict__ pairs, const uint32_t* __restrict__ block_items,
                   const uint32_t* __restrict__ sc_cnt, const uint32_t* __restrict__ sc_base,
                   uint4* __restrict__ csr, unsigned csr_capacity, unsigned coarse_capacity,
                   unsigned long long* __restrict__ hdr, int plan_roles, uint32_t* __restrict__ coarse_count, const uint32_t* __restrict__ block_nvis,
                   const unsigned long long* __restrict__ block_dref, const unsigned long long* __restrict__ feedback,
                   const unsigned long long* __restrict__ dup_pool, unsigned long long* __restrict__ host_out) {
  const int n_scatter = (int)gridDim.x - plan_roles;
  if ((int)blockIdx.x >= n_scatter) {   // uniform per workgroup
    plan_scan_role((int)blockIdx.x - n_scatter, NCB, NB, coarse_count, block_nvis, block_dref, hdr, feedback, dup_pool,
                   host_out, coarse_capacity);
    return;
  }
  const int wg = (int)blockIdx.x;   // scatter workgroup
  __shared__ unsigned s_prefix[SCATTER_BLOCKS + 1];
  __shared__ unsigned s_red[SCATTER_NT / 64 + 1];
  __shared__ unsigned s_delta[SCATTER_BINS];   // first position of the workgroup's run of the bin in `csr` - its first sorted position
  __shared__ unsigned s_cur[SCATTER_BINS];     // the bin's cursor in the sorted order
  __shared__ unsigned short s_idx[SCATTER_IDX];   // pair index at every sorted position
  const int tid = threadIdx.x;
  const int b0 = wg * SCATTER_BLOCKS, nblk = min(SCATTER_BLOCKS, NB - b0);
  const unsigned total = scatter_prefix(block_items, b0, nblk, s_prefix);
  if (total == 0u) return;
  for (int r0 = 0; r0 < NCB; r0 += SCATTER_BINS) {
    const int nbins = min(SCATTER_BINS, NCB - r0);
    // counts -> sorted positions (a thread's four bins are neighbours in that order)
    static_assert(SCATTER_BINS <= 4 * SCATTER_NT, "four bins per thread");
    unsigned c[4], base[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * SCATTER_NT;
      c[u] = i < nbins ? sc_cnt[(size_t)wg * NCB + r0 + i] : 0u;
      base[u] = i < nbins ? sc_base[(size_t)wg * NCB + r0 + i] : 0u;
    }
    unsigned round_total;
    unsigned p = block_excl_scan_u32<SCATTER_NT>(c[0] + c[1] + c[2] + c[3], &round_total, s_red);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * SCATTER_NT;
      if (i < nbins) { s_delta[i] = base[u] - p; s_cur[i] = p; }
      p += c[u];
    }
    __syncthreads();
    // sorted position of every pair; those beyond the index buffer (a workgroup with > 15 360 pairs in this round of bins)
    // are written at once, unsorted
    for (unsigned i0 = tid; i0 < total; i0 += SCATTER_MLP * SCATTER_NT) {
      uint4 it[SCATTER_MLP];
#pragma unroll
      for (int u = 0; u < SCATTER_MLP; ++u)
        it[u] = i0 + u * SCATTER_NT < total ? *scatter_pair(pairs, s_prefix, b0, nblk, i0 + u * SCATTER_NT)
                                            : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int u = 0; u < SCATTER_MLP; ++u) {
        const unsigned m = it[u].w & 0xffffu;
        const int cb = (int)(it[u].w >> 16) - r0;
        if (m && cb >= 0 && cb < nbins) {
          const unsigned pos = atomicAdd(&s_cur[cb], 1u);
          if (pos < (unsigned)SCATTER_IDX) {
            s_idx[pos] = (unsigned short)(i0 + u * SCATTER_NT);
          } else {
            const unsigned at = s_delta[cb] + pos;
            if (at < csr_capacity) csr[at] = make_uint4(it[u].x, it[u].y, it[u].z, m);
            else hdr[HDR_OVERFLOW] = 1ull;   // (cannot happen: the runs hold exactly the pairs that exist)
          }
        }
      }
    }
    __syncthreads();
    const unsigned nsorted = min(round_total, (unsigned)SCATTER_IDX);
    for (unsigned q0 = tid; q0 < nsorted; q0 += SCATTER_MLP * SCATTER_NT) {
      uint4 it[SCATTER_MLP];
#pragma unroll
      for (int u = 0; u < SCATTER_MLP; ++u)
        it[u] = q0 + u * SCATTER_NT < nsorted ? *scatter_pair(pairs, s_prefix, b0, nblk, s_idx[q0 + u * SCATTER_NT])
                                              : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int u = 0; u < SCATTER_MLP; ++u) {
        if (q0 + u * SCATTER_NT < nsorted) {
          const int cb = (int)(it[u].w >> 16) - r0;
          const unsigned at = s_delta[cb] + (q0 + u * SCATTER_NT);
          if (at < csr_capacity) csr[at] = make_uint4(it[u].x, it[u].y, it[u].z, it[u].w & 0xffffu);
          else hdr[HDR_OVERFLOW] = 1ull;
        }
      }
    }
    __syncthreads();
  }
}

// List-slot bases of the coarse bins (one workgroup, any thread count that is a multiple of 64 up to 1024): bin cb's
// tiles will need at most hits(cb) + 16 x 63 slots (every list starts on a multiple of 64), rounded up to 64; the
// exclusive scan over the bins goes into word 2 of the bin's counter line, the total into the header. Replaces a device
// atomic per bin on ONE allocator word in fine_bin (2 040 returning atomics at ~10 ns: 20 of its 61 us).
__device__ void bin_base_scan(int NCB, uint32_t* __restrict__ coarse_count, unsigned long long* __restrict__ hdr) {
  __shared__ unsigned long long bb_wave[17];
  const int nt = blockDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = nt >> 6;
  unsigned long long carry = 0;
  for (int c0 = 0; c0 < NCB; c0 += nt) {
    const int cb = c0 + threadIdx.x;
    const unsigned need = cb < NCB ? bin_slots_needed(coarse_count[(size_t)cb * CC_STRIDE + 1]) : 0u;
    unsigned long long incl = need;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    __syncthreads();
    if (lane == 63) bb_wave[wave] = incl;
    __syncthreads();
    unsigned long long before = carry, all = 0;
    for (int w = 0; w < nw; ++w) { const unsigned long long t = bb_wave[w]; if (w < wave) before += t; all += t; }
    if (cb < NCB) coarse_count[(size_t)cb * CC_STRIDE + 2] = (unsigned)min(before + incl - need, 0xffffffffull);
    carry += all;
  }
  if (threadIdx.x == 0) hdr[HDR_ITEM_ALLOC] = carry;
}

__global__ void __launch_bounds__(1024) bin_base_scan_kernel(int NCB, uint32_t* __restrict__ coarse_count,
                                                            unsigned long long* __restrict__ hdr) {
  bin_base_scan(NCB, coarse_count, hdr);
}

// ------------------------------------------------------------------------------------------------
// K2: single workgroup: counters for the host (visible count, reference duplicate total, fullest coarse bin).
constexpr int SCAN_NT = 1024;
static_assert(SCAN_NT == SCATTER_NT, "the plan's epilogues can ride in the scatter launch");
__device__ void plan_scan_role(int role, int NCB, int NB, uint32_t* __restrict__ coarse_count,
                               const uint32_t* __restrict__ block_nvis, const unsigned long long* __restrict__ block_dref,
                               unsigned long long* __restrict__ hdr, const unsigned long long* __restrict__ feedback,
                               const unsigned long long* __restrict__ dup_pool, unsigned long long* __restrict__ host_out,
                               unsigned coarse_capacity) {
  if (role == 1) { bin_base_scan(NCB, coarse_count, hdr); return; }   // second workgroup, concurrently
  __shared__ unsigned long long s_acc[SCAN_NT / 64];
  unsigned long long nvis = 0, dref = 0, cmax = 0, dmax = 0;
  for (int i = threadIdx.x; i < NB; i += SCAN_NT) { nvis += block_nvis[i]; dref += block_dref[i]; }
  for (int i = threadIdx.x; i < NCB; i += SCAN_NT) {
    const uint2 c01 = *reinterpret_cast<const uint2*>(&coarse_count[(size_t)i * CC_STRIDE]);
    const unsigned in_csr = coarse_count[(size_t)i * CC_STRIDE + 7];
    cmax = max(cmax, (unsigned long long)c01.x);               // all items of the bin: what the sort route is chosen from
    dmax = max(dmax, (unsigned long long)(c01.x - in_csr));    // the directly appended ones: what the slab has to hold
  }
  for (int pass = 0; pass < 4; ++pass) {
    unsigned long long v = pass == 0 ? nvis : pass == 1 ? dref : pass == 2 ? cmax : dmax;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(v, d);
      v = pass >= 2 ? max(v, o) : v + o;
    }
    if (lane_id() == 0) s_acc[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = 0;
      for (int w = 0; w < SCAN_NT / 64; ++w) t = pass >= 2 ? max(t, s_acc[w]) : t + s_acc[w];
      hdr[pass == 0 ? HDR_N_VIS : pass == 1 ? HDR_D_REF : pass == 2 ? HDR_MAX_BIN_ITEMS : HDR_MAX_COARSE] = t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {   // duplicates of the frame = what the pools handed out
    unsigned long long d = 0;
    for (int q = 0; q < DUP_POOLS; ++q) d += dup_pool[q * DP_STRIDE];
    hdr[HDR_D_EFF] = d;
  }
  __syncthreads();
  // publish the first 8 header words straight into the caller's pinned host buffer (fine-grained memory: visible
  // to the host once this kernel has completed) -- the host can then decide about a capacity retry while the render
  // stage is already running, without a copy engine round trip in the middle of the stream
  if (threadIdx.x == 0 && host_out) {
#pragma unroll
    for (int i = 0; i < 8; ++i) host_out[i] = hdr[i];
    // When this role rides in the scatter launch, scatter workgroups may still be about to flag a bin that runs past its
    // slab: the bins' totals are final (bin_rank), so the published overflow word is completed from them
    if (hdr[HDR_MAX_COARSE] > (unsigned long long)coarse_capacity) host_out[HDR_OVERFLOW] = 1ull;
    // words 8..15: this frame's optional-work counts, and the late statistics of the PREVIOUS frame (its render /
    // backward stages completed before this kernel started: same stream) -- what the caller picks launch hints from
    host_out[8] = hdr[HDR_BIG_COUNT];
    host_out[9] = hdr[HDR_BIG_CHUNKS];
    host_out[10] = feedback ? feedback[FB_VALID] : 0ull;
    host_out[11] = feedback ? feedback[FB_LONG_TILES] : 0ull;
    host_out[12] = feedback ? feedback[FB_MAX_LIST] : 0ull;
    host_out[13] = feedback ? feedback[FB_PREFILLED] : 0ull;
    host_out[14] = feedback ? feedback[FB_OVER_512] : 0ull;
    host_out[15] = hdr[HDR_MAX_BIN_ITEMS];
  }
}

// the same two roles as a launch of their own (one-pass binning, SFGS_PLAN_SCAN=separate)
__global__ void __launch_bounds__(SCAN_NT)
plan_scan_kernel(int NCB, int NB, uint32_t* __restrict__ coarse_count, const uint32_t* __restrict__ block_nvis,
                 const unsigned long long* __restrict__ block_dref, unsigned long long* __restrict__ hdr,
                 const unsigned long long* __restrict__ feedback, const unsigned long long* __restrict__ dup_pool,
                 unsigned long long* __restrict__ host_out, unsigned coarse_capacity) {
  plan_scan_role((int)blockIdx.x, NCB, NB, coarse_count, block_nvis, block_dref, hdr, feedback, dup_pool, host_out,
                 coarse_capacity);
}

static bool plan_scan_separate() { return option(OPT_PLAN_SCAN) != 0; }   // the plan's epilogues as a launch of their own (A/B, tests)

int plan_binning(const SfgsFrame* frame, int N, const GeomView& gv, const TilesView& tv, const BinsView& bv,
                 int64_t coarse_capacity, bool two_pass, void* counters_pinned_host, hipStream_t stream) {
  const int64_t NCB = coarse_bins(frame->image_width, frame->image_height);
  const int NB = (int)pre_blocks(N);
  int plan_roles = 0;   // 2: the plan's epilogues ride in the scatter launch (two-pass binning)
  if (NB > 0) {
    if (two_pass) {
      const int NWG = (int)scatter_groups(N);
      { ProfScope ps_(KID_BIN_COUNT, stream);
        hipLaunchKernelGGL(bin_count_kernel, dim3(NWG), dim3(SCATTER_NT), 0, stream, NB, (int)NCB, bv.pairs,
                           gv.block_items, tv.sc_cnt, tv.sc_hits); }
      { ProfScope ps_(KID_BIN_RANK, stream);
        hipLaunchKernelGGL(bin_rank_kernel, dim3(((int)NCB + RANK_COLS - 1) / RANK_COLS), dim3(RANK_COLS * RANK_GROUPS), 0,
                           stream, NWG, (int)NCB, tv.sc_cnt, tv.sc_hits, tv.sc_base, tv.coarse_count, tv.hdr); }
      plan_roles = plan_scan_separate() ? 0 : 2;
      { ProfScope ps_(KID_BIN_SCATTER, stream);
        hipLaunchKernelGGL(bin_scatter_kernel, dim3(NWG + plan_roles), dim3(SCATTER_NT), 0, stream, NB, (int)NCB, bv.pairs,
                           gv.block_items, tv.sc_cnt, tv.sc_base, bv.csr,
                           (unsigned)std::min<size_t>(pairs_bytes(N) / 16, 0xffffffffull), (unsigned)coarse_capacity, tv.hdr, plan_roles,
                           tv.coarse_count, tv.block_nvis, tv.block_dref, (const unsigned long long*)frame->feedback,
                           (const unsigned long long*)tv.dup_pool, (unsigned long long*)counters_pinned_host); }
    }
    SFGS_POST_LAUNCH("bin_scatter", stream, frame->debug);
  }
  if (plan_roles == 0)
  { ProfScope ps_(KID_PLAN_SCAN, stream);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(2), dim3(SCAN_NT), 0, stream, (int)NCB, NB, tv.coarse_count, tv.block_nvis,
                       tv.block_dref, tv.hdr,
                       (const unsigned long long*)frame->feedback, (const unsigned long long*)tv.dup_pool,
                       (unsigned long long*)counters_pinned_host, (unsigned)coarse_capacity); }
  SFGS_POST_LAUNCH("plan_scan", stream, frame->debug);
  return SFGS_OK;
}

}  // namespace sfgs

using namespace sfgs;

// ------------------------------------------------------------------------------------------------
// Joint render with the GAUSSIANS sharded over ranks: every rank plans its own Gaussians, EXPORTS the plan's
// per-Gaussian records and per-coarse-bin items in a layout that can be all-gathered (fixed strides), and MERGES the
// gathered parts into one plan whose Gaussian ids are the positions in the concatenated set -- the render stage then
// bins, sorts (by depth bits, then id: the single-process order) and composites this rank's band.
constexpr int MERGE_MAX_PARTS = 16;
struct MergeParts {
  const float4* rec[MERGE_MAX_PARTS];
  const uint32_t* count[MERGE_MAX_PARTS];
  const uint4* items[MERGE_MAX_PARTS];
  unsigned base[MERGE_MAX_PARTS + 1];   // first merged id of every part
  int parts;
};

__global__ void __launch_bounds__(256)
plan_export_kernel(int N, int NCB, const float4* __restrict__ rec, const uint32_t* __restrict__ coarse_count,
                   const uint4* __restrict__ csr, const uint4* __restrict__ slabs, unsigned coarse_capacity,
                   unsigned export_capacity, float4* __restrict__ rec_out, uint32_t* __restrict__ count_out,
                   uint4* __restrict__ items_out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
  for (size_t i = t; i < (size_t)N * 3; i += nthreads) rec_out[i] = rec[(i / 3) * REC_F4 + i % 3];
  for (size_t cb = t; cb < (size_t)NCB; cb += nthreads)
    count_out[cb] = min(bin_items(coarse_count + cb * CC_STRIDE, csr, slabs, cb, coarse_capacity).n, export_capacity);
  for (size_t i = t; i < (size_t)NCB * export_capacity; i += nthreads) {
    const size_t cb = i / export_capacity, k = i % export_capacity;
    const BinItems b = bin_items(coarse_count + cb * CC_STRIDE, csr, slabs, cb, coarse_capacity);
    if (k < b.n) items_out[i] = b[(unsigned)k];
  }
}

__global__ void __launch_bounds__(256)
plan_merge_rec_kernel(MergeParts mp, float4* __restrict__ rec) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
  for (int p = 0; p < mp.parts; ++p) {
    const size_t n = (size_t)(mp.base[p + 1] - mp.base[p]) * 3;
    for (size_t i = t; i < n; i += nthreads) rec[((size_t)mp.base[p] + i / 3) * REC_F4 + i % 3] = mp.rec[p][i];
  }
}

// one workgroup per coarse bin: the parts' items one after the other (part order = id order), ids re-based
__global__ void __launch_bounds__(256)
plan_merge_items_kernel(MergeParts mp, unsigned export_capacity, unsigned coarse_capacity,
                        uint32_t* __restrict__ coarse_count, uint4* __restrict__ slabs, unsigned long long* __restrict__ hdr) {
  __shared__ unsigned s_hits[4];
  const size_t cb = blockIdx.x;
  unsigned off = 0, hits = 0;
  for (int p = 0; p < mp.parts; ++p) {
    const unsigned n = min(mp.count[p][cb], export_capacity);
    for (unsigned k = threadIdx.x; k < n; k += 256) {
      uint4 it = mp.items[p][cb * export_capacity + k];
      it.x += mp.base[p];
      it.z = 0u;            // duplicate indices belong to the backward: a merged plan is rendered, not differentiated
      if (off + k < coarse_capacity) slabs[cb * coarse_capacity + off + k] = it;
      hits += (unsigned)__popc(it.w);
    }
    off += n;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) hits += (unsigned)__shfl_xor((int)hits, d);
  if ((threadIdx.x & 63) == 0) s_hits[threadIdx.x >> 6] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    coarse_count[cb * CC_STRIDE] = off;
    coarse_count[cb * CC_STRIDE + 1] = s_hits[0] + s_hits[1] + s_hits[2] + s_hits[3];   // tile hits: list-slot need
    if (off > coarse_capacity) hdr[HDR_OVERFLOW] = 1ull;
  }
}

extern "C" int sfgs_raster_plan_export(const SfgsFrame* frame, int32_t N, const void* geom, const void* tiles,
                                       const void* bins, int64_t dup_capacity, int64_t coarse_capacity,
                                       int64_t export_capacity, float* rec_out, uint32_t* count_out, void* items_out,
                                       void* stream_) {
  if (int rc = check_frame(frame)) return rc;
  SFGS_REQUIRE(N >= 0 && geom && tiles && bins && count_out && items_out && (N == 0 || rec_out), SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(export_capacity > 0 && export_capacity < (1ll << 31) && coarse_capacity >= 0, SFGS_E_ARG, "bad capacity");
  hipStream_t stream = (hipStream_t)stream_;
  const int W = frame->image_width, H = frame->image_height;
  const int64_t NCB = coarse_bins(W, H);
  const TilesView tv = tiles_view(const_cast<void*>(tiles), W, H, N, nullptr);
  const GeomView gv = geom_view(const_cast<void*>(geom), N);
  const BinsView bv = bins_view_csr(const_cast<void*>(bins), dup_capacity, NCB, coarse_capacity, N);
  hipLaunchKernelGGL(plan_export_kernel, dim3(2048), dim3(256), 0, stream, (int)N, (int)NCB, gv.rec, tv.coarse_count,
                     bv.csr, bv.slabs, (unsigned)coarse_capacity, (unsigned)export_capacity, (float4*)rec_out, count_out,
                     (uint4*)items_out);
  SFGS_POST_LAUNCH("plan_export", stream, frame->debug);
  return SFGS_OK;
}

extern "C" int sfgs_raster_plan_merge(const SfgsFrame* frame, int32_t parts, const int32_t* part_N,
                                      const float* const* part_rec, const uint32_t* const* part_count,
                                      const void* const* part_items, int64_t export_capacity, void* geom, size_t geom_sz,
                                      void* tiles, size_t tiles_sz, void* bins, size_t bins_sz, int64_t dup_capacity,
                                      int64_t coarse_capacity, void* stream_) {
  if (int rc = check_frame(frame)) return rc;
  SFGS_REQUIRE(parts >= 1 && parts <= MERGE_MAX_PARTS, SFGS_E_ARG, "1..%d parts", MERGE_MAX_PARTS);
  SFGS_REQUIRE(part_N && part_rec && part_count && part_items && geom && tiles && bins, SFGS_E_ARG, "NULL argument");
  SFGS_REQUIRE(export_capacity > 0 && export_capacity < (1ll << 31), SFGS_E_ARG, "bad export_capacity");
  hipStream_t stream = (hipStream_t)stream_;
  const int W = frame->image_width, H = frame->image_height;
  const int64_t NCB = coarse_bins(W, H);
  MergeParts mp;
  int64_t N = 0;
  for (int p = 0; p < parts; ++p) {
    SFGS_REQUIRE(part_N[p] >= 0 && part_count[p] && part_items[p] && (part_N[p] == 0 || part_rec[p]), SFGS_E_ARG, "bad part %d", p);
    mp.rec[p] = (const float4*)part_rec[p]; mp.count[p] = part_count[p]; mp.items[p] = (const uint4*)part_items[p];
    mp.base[p] = (unsigned)N;
    N += part_N[p];
  }
  mp.base[parts] = (unsigned)N;
  mp.parts = parts;
  SFGS_REQUIRE(N < (1ll << 31), SFGS_E_ARG, "too many Gaussians");
  size_t tb = 0;
  const TilesView tv = tiles_view(tiles, W, H, N, &tb);
  SFGS_REQUIRE(tiles_sz >= tb, SFGS_E_CAPACITY, "tiles blob: %zu bytes given, %zu needed", tiles_sz, tb);
  SFGS_REQUIRE(geom_sz >= geom_bytes(N), SFGS_E_CAPACITY, "geom blob: %zu bytes given, %zu needed", geom_sz, geom_bytes(N));
  SFGS_REQUIRE(dup_capacity >= 0 && dup_capacity < (1ll << 32) && coarse_capacity >= 0 && coarse_capacity < (1ll << 31),
               SFGS_E_ARG, "bad dup_capacity / coarse_capacity");
  // (the plan-sized blob: the render stage reads the bin-sorted items of the two-pass binning, which lie at its END)
  SFGS_REQUIRE(bins_sz >= bins_bytes_plan(dup_capacity, NCB, coarse_capacity, N), SFGS_E_CAPACITY,
               "bins blob: %zu bytes given, %zu needed (the blob the plan was given: sfgs_raster_sizes().bins_bytes)", bins_sz,
               bins_bytes_plan(dup_capacity, NCB, coarse_capacity, N));
  const GeomView gv = geom_view(geom, N);
  const BinsView bv = bins_view(bins, dup_capacity, NCB, coarse_capacity);
  SFGS_CHECK_HIP(zero_head(tiles, tv.zero_bytes, stream));
  if (frame->subpixel_offset) launch_subpix_bound(frame->subpixel_offset, W, H, tv.hdr, stream);
  if (N > 0) hipLaunchKernelGGL(plan_merge_rec_kernel, dim3(2048), dim3(256), 0, stream, mp, gv.rec);
  hipLaunchKernelGGL(plan_merge_items_kernel, dim3((unsigned)NCB), dim3(256), 0, stream, mp, (unsigned)export_capacity,
                     (unsigned)coarse_capacity, tv.coarse_count, bv.slabs, tv.hdr);
  hipLaunchKernelGGL(bin_base_scan_kernel, dim3(1), dim3(1024), 0, stream, (int)NCB, tv.coarse_count, tv.hdr);
  SFGS_POST_LAUNCH("plan_merge", stream, frame->debug);
  return SFGS_OK;
}
