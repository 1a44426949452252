// raster_sort.hip -- first stage of the forward's render (map of the forward: raster_fwd.hip): from the coarse bins'
// items to every 8x8 tile's list of Gaussian ids, front to back. Two routes, bit-identical lists:
//   split:  fine_bin (per coarse bin: LDS-ranked expansion into per-tile item segments) -> sort_tiles_reg (lists up to
//           512 entries: normalised bitonic network in registers);
//   fused:  select_sort (both in one kernel, no per-tile items in memory; lists up to 512 / 768 / 1 024 entries, on one
//           exact 32-bit word per entry where a tile allows it);
// and behind either the long lists: sort_tiles_reg_long (513 .. 1 024 entries, 16 keys per lane) and sort_tiles_long
// (bucketed sort, LDS network, LDS/global hybrid), or sort_tiles_long alone under the FEW_LONG_LISTS hint.
#include <algorithm>
#include <type_traits>

#include "sfgs_internal.h"

namespace sfgs {

constexpr int REG_SORT_SMALL = 512;  // lists up to here: sort_tiles_reg_kernel (<= 8 keys per lane, 8 waves per SIMD)
constexpr int REG_SORT_MAX = 1024;   // lists up to here: register network too (16 keys per lane), separate kernel

// ------------------------------------------------------------------------------------------------
// K3: fine binning. One 256-thread workgroup per coarse bin: count the bin's 16 tiles with LDS atomics,
// reserve the bin's list slots with ONE device atomic, publish (start, length) of its tiles, then expand
// every coarse item into its per-tile duplicates: items[slot] = (id, depth, dup index, 0).
__global__ void __launch_bounds__(256)
fine_bin_kernel(int TX8, int TY8, int CX, int NCB, const uint32_t* __restrict__ coarse_count,
                const uint4* __restrict__ csr, const uint4* __restrict__ slabs, unsigned coarse_capacity,
                unsigned long long slot_capacity,
                uint2* __restrict__ tile_range, uint4* __restrict__ items, uint32_t* __restrict__ long_tiles,
                unsigned long long* __restrict__ hdr) {
  __shared__ unsigned cnt[COARSE_TILES];
  __shared__ unsigned long long s_base;
  const int cb = blockIdx.x, tid = threadIdx.x;
  const BinItems slab = bin_items(coarse_count + (size_t)cb * CC_STRIDE, csr, slabs, (size_t)cb, coarse_capacity);
  const unsigned n = slab.n;
  if (tid < COARSE_TILES) cnt[tid] = 0;
  __syncthreads();
  // the bin's coarse items are read ONCE, all loads of a thread in flight together (the kernel is latency-bound: one
  // round of workgroups, each a chain of dependent global loads and LDS atomics); bins with more than 256 * FB_R items
  // take the remainder from memory in both passes
  constexpr int FB_R = 12;
  uint4 reg[FB_R];
  // UNCONDITIONAL loads from a clamped index, the tile mask cleared afterwards: written as `i < n ? slab[i] : 0` every
  // load sat in its own exec-masked block with an s_waitcnt vmcnt(0) right behind it -- twelve serialised round trips to
  // memory per workgroup instead of one (found by reading the ISA, round 3)
  const unsigned last = n ? n - 1u : 0u;
#pragma unroll
  for (int k = 0; k < FB_R; ++k) reg[k] = slab[min(tid + 256u * k, last)];
#pragma unroll
  for (int k = 0; k < FB_R; ++k)
    if (tid + 256u * k >= n) reg[k].w = 0u;
#pragma unroll
  for (int k = 0; k < FB_R; ++k) {
    unsigned m = reg[k].w;
    while (m) { const int b = __builtin_ctz(m); m &= m - 1; atomicAdd(&cnt[b], 1u); }
  }
  for (unsigned i = tid + 256u * FB_R; i < n; i += 256) {
    unsigned m = slab[i].w;
    while (m) { const int b = __builtin_ctz(m); m &= m - 1; atomicAdd(&cnt[b], 1u); }
  }
  __syncthreads();
  if (tid < 64) {  // first wave: exclusive scan of the 16 counts, one allocation for the whole bin
    const unsigned c = tid < COARSE_TILES ? cnt[tid] : 0u;
    // every list starts on a multiple of LIST_ALIGN (= 64) slots: the compositing kernels load ids 64 at a time from
    // 256-byte aligned addresses, and slot s + 64 b + lane doubles as the index of the per-pixel hit-mask word of the
    // tile's b-th batch (image blob). Costs index space only (<= 63 unused slots per tile), no traffic.
    const unsigned ca = (c + LIST_ALIGN - 1) & ~(unsigned)(LIST_ALIGN - 1);
    unsigned incl = ca;
#pragma unroll
    for (int d = 1; d < COARSE_TILES; d <<= 1) { const unsigned t = __shfl_up(incl, d); if (tid >= d) incl += t; }
    const unsigned total = __shfl(incl, COARSE_TILES - 1);
    unsigned long long base = 0;
    if (tid == 0) {
      // the bin's first list slot: scanned by the plan from the bins' tile-hit totals (an upper bound of what the bin's
      // lists take: `total` <= hits + 16 x 63), no allocator atomic
      base = coarse_count[(size_t)cb * CC_STRIDE + 2];
      // memory safety when the caller's slot capacity is too small (the wrapper sizes it with
      // sfgs_raster_slot_capacity, which always suffices): the bin's lists are dropped and the frame is flagged
      if (base + total > slot_capacity) { hdr[HDR_OVERFLOW] = 1ull; base = ~0ull; }
      s_base = base;
    }
    base = __shfl(base, 0);
    const bool dropped = base == ~0ull;
    const unsigned off = incl - ca;
    if (tid < COARSE_TILES) {
      const int tx = (cb % CX) * COARSE + (tid & (COARSE - 1)), ty = (cb / CX) * COARSE + (tid / COARSE);
      if (tx < TX8 && ty < TY8) {
        tile_range[ty * TX8 + tx] = dropped ? make_uint2(0u, 0u) : make_uint2((unsigned)base + off, c);
        if (c > REG_SORT_SMALL && !dropped) long_tiles[atomicAdd(&hdr[HDR_LONG_COUNT], 1ull)] = (unsigned)(ty * TX8 + tx);  // rare
      }
      cnt[tid] = off;  // becomes the per-tile cursor
    }
    {  // longest list of the bin: ONE atomic per workgroup (16 same-address atomics per bin serialise in the L2)
      unsigned cm = tid < COARSE_TILES ? c : 0u;
#pragma unroll
      for (int d = 8; d >= 1; d >>= 1) cm = max(cm, (unsigned)__shfl_xor((int)cm, d));
      if (tid == 0 && cm) atomicMax((unsigned int*)&hdr[HDR_MAX_LIST], cm);
    }
  }
  __syncthreads();
  const unsigned long long base = s_base;
  if (base == ~0ull) return;
  auto expand = [&](const uint4 it) {
    unsigned m = it.w, dup = it.z;
    while (m) {
      const int b = __builtin_ctz(m);
      m &= m - 1;
      const unsigned slot = atomicAdd(&cnt[b], 1u);
      items[base + slot] = make_uint4(it.x, it.y, dup, 0u);
      ++dup;
    }
  };
#pragma unroll
  for (int k = 0; k < FB_R; ++k) expand(reg[k]);
  for (unsigned i = tid + 256u * FB_R; i < n; i += 256) expand(slab[i]);
}

// ------------------------------------------------------------------------------------------------
// K4a: per-tile sort for lists of up to 512 entries, entirely in registers. One wave per tile; element
// (lane, r) of the wave carries label e = lane * EPL + r. Normalised bitonic network: for every size the
// first step pairs e with e ^ (size - 1), the following steps with e ^ stride; the lower label keeps the
// smaller key. Label bits below log2(EPL) are register indices (compile-time), the bits above are lane
// bits: those exchanges are cross-lane shuffles (3 per element: key hi/lo + payload). No LDS traffic, no
// bank conflicts, no barriers. Keys: (depth bits << 32 | Gaussian id) == SURVEY A.3 order.
// value of lane (l ^ K): DPP where the hardware has the permutation (no LDS latency), the LDS crossbar
// (ds_swizzle / ds_bpermute) otherwise.
template <int K>
__device__ __forceinline__ unsigned xor_shuffle(unsigned v) {
  if constexpr (K == 1) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);       // quad_perm [1,0,3,2]
  else if constexpr (K == 2) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
  else if constexpr (K == 3) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x1B, 0xf, 0xf, false);  // quad_perm [3,2,1,0]
  else if constexpr (K == 7) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false); // row_half_mirror
  else if constexpr (K == 15) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false); // row_mirror
  else if constexpr (K < 32) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, (K << 10) | 0x1f);           // bit mode: xor K
  else return (unsigned)__shfl_xor((int)v, K);
}

template <int EPL, int SIZE, int STEP>
__device__ __forceinline__ void bitonic_stage(unsigned long long (&key)[EPL], unsigned (&pay)[EPL], int lane) {
  constexpr int mask = STEP == 0 ? SIZE - 1 : (SIZE >> (STEP + 1));
  constexpr int rmask = mask & (EPL - 1);   // register-index part of the label
  constexpr int lmask = mask / EPL;         // lane part
  if constexpr (lmask == 0) {
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      const int q = r ^ rmask;
      if (q > r) {
        const bool sw = key[q] < key[r];
        const unsigned long long kr = key[r], kq = key[q];
        const unsigned pr = pay[r], pq = pay[q];
        key[r] = sw ? kq : kr; key[q] = sw ? kr : kq;
        pay[r] = sw ? pq : pr; pay[q] = sw ? pr : pq;
      }
    }
  } else {
    const bool upper = (lane & (lmask & ~(lmask >> 1))) != 0;  // highest bit of the mask decides who is lower
    unsigned long long nk[EPL];
    unsigned np[EPL];
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      const int q = r ^ rmask;  // partner's register index
      const unsigned hi = xor_shuffle<lmask>((unsigned)(key[q] >> 32));
      const unsigned lo = xor_shuffle<lmask>((unsigned)(key[q] & 0xffffffffull));
      const unsigned pp = xor_shuffle<lmask>(pay[q]);
      const unsigned long long theirs = ((unsigned long long)hi << 32) | lo;
      const bool take = (theirs < key[r]) != upper;  // the lower label keeps the minimum, the upper the maximum
      nk[r] = take ? theirs : key[r];
      np[r] = take ? pp : pay[r];
    }
#pragma unroll
    for (int r = 0; r < EPL; ++r) { key[r] = nk[r]; pay[r] = np[r]; }
  }
}

template <int EPL, int SIZE, int STEP>
__device__ __forceinline__ void bitonic_steps(unsigned long long (&key)[EPL], unsigned (&pay)[EPL], int lane) {
  if constexpr (STEP == 0 || (SIZE >> (STEP + 1)) >= 1) {
    bitonic_stage<EPL, SIZE, STEP>(key, pay, lane);
    bitonic_steps<EPL, SIZE, STEP + 1>(key, pay, lane);
  }
}

template <int EPL, int SIZE>
__device__ __forceinline__ void bitonic_sizes(unsigned long long (&key)[EPL], unsigned (&pay)[EPL], int lane) {
  if constexpr (SIZE <= 64 * EPL) {
    bitonic_steps<EPL, SIZE, 0>(key, pay, lane);
    bitonic_sizes<EPL, SIZE * 2>(key, pay, lane);
  }
}

template <int EPL>
__device__ __forceinline__ void wave_bitonic_sort(unsigned long long (&key)[EPL], unsigned (&pay)[EPL], int lane) {
  bitonic_sizes<EPL, 2>(key, pay, lane);
}

// The same network on ONE 32-bit word per element (select_sort_kernel's exact tile-relative key, raster_math.h: sortkey_pack;
// the word carries the entry's list position, so nothing travels with it): an in-register pair is v_min_u32 + v_max_u32, a
// cross-lane exchange one shuffle instead of three. Equal words only occur among the padding, where either choice is the same.
template <int EPL, int SIZE, int STEP>
__device__ __forceinline__ void bitonic_stage(unsigned (&key)[EPL], int lane) {
  constexpr int mask = STEP == 0 ? SIZE - 1 : (SIZE >> (STEP + 1));
  constexpr int rmask = mask & (EPL - 1);
  constexpr int lmask = mask / EPL;
  if constexpr (lmask == 0) {
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      const int q = r ^ rmask;
      if (q > r) {
        const unsigned kr = key[r], kq = key[q];
        key[r] = min(kr, kq); key[q] = max(kr, kq);
      }
    }
  } else {
    const bool upper = (lane & (lmask & ~(lmask >> 1))) != 0;
    unsigned nk[EPL];
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      const unsigned theirs = xor_shuffle<lmask>(key[r ^ rmask]);
      nk[r] = upper ? max(key[r], theirs) : min(key[r], theirs);
    }
#pragma unroll
    for (int r = 0; r < EPL; ++r) key[r] = nk[r];
  }
}

template <int EPL, int SIZE, int STEP>
__device__ __forceinline__ void bitonic_steps(unsigned (&key)[EPL], int lane) {
  if constexpr (STEP == 0 || (SIZE >> (STEP + 1)) >= 1) {
    bitonic_stage<EPL, SIZE, STEP>(key, lane);
    bitonic_steps<EPL, SIZE, STEP + 1>(key, lane);
  }
}

template <int EPL, int SIZE>
__device__ __forceinline__ void bitonic_sizes(unsigned (&key)[EPL], int lane) {
  if constexpr (SIZE <= 64 * EPL) {
    bitonic_steps<EPL, SIZE, 0>(key, lane);
    bitonic_sizes<EPL, SIZE * 2>(key, lane);
  }
}

template <int EPL>
__device__ __forceinline__ void wave_bitonic_sort(unsigned (&key)[EPL], int lane) {
  bitonic_sizes<EPL, 2>(key, lane);
}

// smallest value of the wave, in every lane (uniform): DPP inside a row of 16 lanes, one readlane per row
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  v = min(v, xor_shuffle<1>(v));
  v = min(v, xor_shuffle<2>(v));
  v = min(v, xor_shuffle<7>(v));    // row_half_mirror: the other quad of the lane's group of 8
  v = min(v, xor_shuffle<15>(v));   // row_mirror: the other group of 8
  const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
  const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
  return min(min(a, b), min(c, d));
}

// A lane's EPL consecutive list entries (positions lane * EPL ..) as 16-byte (8- / 4-byte) stores instead of EPL dword
// stores 4 * EPL bytes apart (round 4: one scattered dword store per entry was the expensive way to write a list, cf.
// profiles/r4_bwd_store3_ab.txt). Every list owns its slots up to the next multiple of 64 (LIST_ALIGN), so a lane whose
// group starts inside that range writes all of it; the entries beyond the list's length are padding nobody reads.
template <int EPL>
__device__ __forceinline__ void store_list_entries(uint32_t* __restrict__ dst, const unsigned (&v)[EPL]) {
  if constexpr (EPL >= 4) {
#pragma unroll
    for (int i = 0; i < EPL / 4; ++i)
      reinterpret_cast<uint4*>(dst)[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else if constexpr (EPL == 2) {
    *reinterpret_cast<uint2*>(dst) = make_uint2(v[0], v[1]);
  } else {
    dst[0] = v[0];
  }
}

template <int EPL>
__device__ __forceinline__ void sort_tile_in_registers(unsigned s, int L, int lane, const uint4* __restrict__ items,
                                                       uint32_t* __restrict__ sorted_id,
                                                       uint32_t* __restrict__ sorted_dup) {
  unsigned long long key[EPL];
  unsigned pay[EPL];
  // coalesced (striped) loads, all in flight together: unconditional from a clamped index, padding selected afterwards
  // (a load under `if (i < L)` gets its own exec-masked block and, every few of them, an s_waitcnt vmcnt(0))
  uint4 it[EPL];
#pragma unroll
  for (int r = 0; r < EPL; ++r) it[r] = items[s + min(r * 64 + lane, L - 1)];
#pragma unroll
  for (int r = 0; r < EPL; ++r) {   // the network sorts any initial arrangement
    const bool in = r * 64 + lane < L;
    key[r] = in ? (((unsigned long long)it[r].y << 32) | it[r].x) : ~0ull;
    pay[r] = in ? it[r].z : 0u;
  }
  wave_bitonic_sort<EPL>(key, pay, lane);
  static_assert(LIST_ALIGN % EPL == 0, "a lane's entries lie inside or outside the list's slot range as a whole");
  if (lane * EPL < ((L + LIST_ALIGN - 1) & ~(LIST_ALIGN - 1))) {
    unsigned ids[EPL];
#pragma unroll
    for (int r = 0; r < EPL; ++r) ids[r] = (unsigned)(key[r] & 0xffffffffull);
    store_list_entries<EPL>(sorted_id + s + lane * EPL, ids);
    store_list_entries<EPL>(sorted_dup + s + lane * EPL, pay);
  }
}

__global__ void __launch_bounds__(256)
sort_tiles_reg_kernel(int T8, const uint2* __restrict__ tile_range, const uint4* __restrict__ items,
                      uint32_t* __restrict__ sorted_id, uint32_t* __restrict__ sorted_dup,
                      const unsigned long long* __restrict__ hdr, unsigned long long* __restrict__ feedback) {
  if (feedback && blockIdx.x == 0 && threadIdx.x == 0) {   // the list statistics are final (fine_bin has run): leave
    feedback[FB_VALID] = 1ull;                              // them for the next frame's plan (SfgsFrame.feedback)
    feedback[FB_LONG_TILES] = hdr[HDR_LONG_COUNT];
    feedback[FB_MAX_LIST] = hdr[HDR_MAX_LIST];
    feedback[FB_OVER_512] = hdr[HDR_LONG_COUNT];           // this route lists exactly the tiles beyond 512 entries
  }
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= T8) return;
  const uint2 tr = tile_range[t];
  const int L = (int)tr.y;
  if (L == 0 || L > REG_SORT_SMALL) return;
  if (L <= 64) sort_tile_in_registers<1>(tr.x, L, lane, items, sorted_id, sorted_dup);
  else if (L <= 128) sort_tile_in_registers<2>(tr.x, L, lane, items, sorted_id, sorted_dup);
  else if (L <= 256) sort_tile_in_registers<4>(tr.x, L, lane, items, sorted_id, sorted_dup);
  else sort_tile_in_registers<8>(tr.x, L, lane, items, sorted_id, sorted_dup);
}

// K3+K4a fused (round 3): SELECT + SORT, no per-tile item round trip through memory.
// fine_bin expands the coarse items of a bin into 16-byte per-tile items in memory (111 MB written at the headline
// scene) which the sort kernel reads straight back. Here a workgroup takes one ROW of four tiles of a coarse bin (wave =
// tile): it reads the bin's slab once (21 KB on average; the bin's four workgroups are XCD-contiguous and share the L2),
// hands every coarse item to the wave-private LDS lists of the row's tiles its mask names (12 bytes per entry: key =
// depth bits << 32 | id, payload = duplicate index = the item's first index + the mask bits below the tile's; positions
// from LDS atomics -- the order inside a list does not matter before the sort), then every wave sorts its list with the
// register network and writes ids / duplicate indices in their final order. The tile's first slot inside the bin's slot
// range (the plan's scan, bin_slots_needed) comes from one atomic per tile on the bin's OWN counter line (word 3: a cursor
// in units of slots, 16 atomics per line; placement only -- which tile of a bin sits where never reaches a result). Lists
// beyond REG_SORT_SMALL entries (rare) are written out as unsorted items by a second scan of the tile's wave and left to
// the long-list kernels, exactly as fine_bin leaves them. The longest list of the frame is collected per bin (word 4 of
// the line) and reduced by list_stats.
// SS_CAP = entries a tile's LDS list holds = the longest list sorted here: 512 (24 KB of LDS per workgroup, <= 8 keys
// per lane: the SHORT_LISTS form) or 1 024 (round 4: 48 KB, three workgroups per CU, the 16-key network for the lists
// beyond 512 -- the MEDIUM_LISTS form for frames whose lists reach 513..1 024 entries, e.g. the reference's 45 / 25 degree
// IDU cameras (arguments/__init__.py:238-249), which otherwise fell back to fine_bin + two sort kernels).
// (A wave-level LDS radix sort for the lists beyond 256 entries was built and measured in round 4 -- slower below ~700
// entries, not kept: profiles/r4_radix_sort_ab_not_kept.txt.)
// One entry = 12 bytes, as (id, duplicate index) pair + depth bits in arrays of their own: the 32-bit-key sort reads the depths
// alone and fetches the pair of a sorted entry with one 8-byte read.
template <int SS_CAP>
struct alignas(16) SelectSortLds {
  uint2 idp[SS_CAP];        // (Gaussian id, duplicate index)
  uint32_t depth[SS_CAP];   // view depth bits
  uint32_t pad_[4];
};


template <int SS_CAP>
__global__ void __launch_bounds__(256)
select_sort_kernel(int TX8, int TY8, int CX, int NCB, uint32_t* __restrict__ coarse_count,
                   const uint4* __restrict__ csr, const uint4* __restrict__ slabs, unsigned coarse_capacity,
                   unsigned long long slot_capacity,
                   uint2* __restrict__ tile_range, uint4* __restrict__ items, uint32_t* __restrict__ long_tiles,
                   unsigned long long* __restrict__ hdr, uint32_t* __restrict__ sorted_id,
                   uint32_t* __restrict__ sorted_dup, int narrow) {
  __shared__ SelectSortLds<SS_CAP> lds_all[COARSE];
  __shared__ unsigned s_cnt[COARSE];
  // workgroup = one row of four tiles of a coarse bin (wave = tile); the four workgroups of a bin are neighbours on one XCD
  // (chunks of 8 bins = 32 workgroups per XCD turn, dealt round-robin: balanced on frames whose bins are not equally full)
  const unsigned lb = xcd_chunked(blockIdx.x, (unsigned)NCB * COARSE, 8u * COARSE);
  const int cb = (int)(lb / COARSE), q = (int)(lb % COARSE);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int tx = (cb % CX) * COARSE + wave, ty = (cb / CX) * COARSE + q;
  if (ty >= TY8) return;                             // the whole row lies below the image (uniform per workgroup)
  const int t = ty * TX8 + tx;
  const int bit = q * COARSE + wave;                 // this tile's bit of the coarse items' masks
  uint32_t* line = coarse_count + (size_t)cb * CC_STRIDE;
  const BinItems slab = bin_items(line, csr, slabs, (size_t)cb, coarse_capacity);
  const unsigned n = slab.n;
  if (n == 0) { if (lane == 0 && tx < TX8) tile_range[t] = make_uint2(0u, 0u); return; }   // uniform per workgroup
  SelectSortLds<SS_CAP>& lds = lds_all[wave];
  // ---- scan: the workgroup reads the slab ONCE (R items per thread and round trip, unconditional loads from clamped
  // indices) and hands every item to the lists of the row's tiles it touches. Positions come from LDS atomics: the order
  // inside a list is irrelevant here, the sort below fixes it ((depth, id) keys are unique within a tile).
  if (tid < COARSE) s_cnt[tid] = 0u;
  __syncthreads();
  constexpr int R = 8;
  const unsigned rowmask = 0xfu << (q * COARSE);
  for (unsigned i0 = 0; i0 < n; i0 += 256u * R) {
    uint4 it[R];
#pragma unroll
    for (int k = 0; k < R; ++k) it[k] = slab[min(i0 + 256u * k + tid, n - 1u)];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      unsigned m = i0 + 256u * k + tid < n ? it[k].w & rowmask : 0u;
      while (m) {
        const int b = __builtin_ctz(m);
        m &= m - 1;
        const unsigned pos = atomicAdd(&s_cnt[b - q * COARSE], 1u);
        if (pos < (unsigned)SS_CAP) {
          SelectSortLds<SS_CAP>& dst = lds_all[b - q * COARSE];
          dst.depth[pos] = it[k].y;
          dst.idp[pos] = make_uint2(it[k].x, it[k].z + (unsigned)__popc(it[k].w & ((1u << b) - 1u)));
        }
      }
    }
  }
  __syncthreads();
  if (tx >= TX8) return;                             // a tile right of the image: no item has its bit
  const unsigned below = (1u << bit) - 1u;
  const unsigned c = __builtin_amdgcn_readfirstlane((int)s_cnt[wave]);
  // ---- the tile's slots: a stretch of the bin's range (scanned by the plan from the bin's tile hits) ---------------
  const unsigned long long bin_base = line[2];
  const unsigned need = bin_slots_needed(line[1]);
  const bool dropped = bin_base + need > slot_capacity;   // the caller's slot capacity is too small (see fine_bin)
  unsigned off = 0;
  if (lane == 0) {
    if (dropped) hdr[HDR_OVERFLOW] = 1ull;
    else if (c) {
      off = atomicAdd(&line[3], (c + LIST_ALIGN - 1) & ~(unsigned)(LIST_ALIGN - 1));
      atomicMax(&line[4], c);
      if (c > (unsigned)REG_SORT_SMALL) atomicAdd(&line[5], 1u);   // how many of the frame's lists need the 1 024 form
    }
  }
  if (dropped || c == 0) { if (lane == 0) tile_range[t] = make_uint2(0u, 0u); return; }
  if (c <= (unsigned)SS_CAP) {
    // sort first, then address: the returning atomic is only needed by the stores behind the sort
    const int L = (int)c;
    auto finish = [&](auto epl_tag) {
      constexpr int EPL = decltype(epl_tag)::value;
      const bool owns = lane * EPL < ((L + LIST_ALIGN - 1) & ~(LIST_ALIGN - 1));   // the tile owns its slots up to the next multiple of 64
      if (narrow) {
        // ---- one exact 32-bit word per entry (raster_math.h: sortkey_*): depth bits relative to the tile's nearest entry above
        // the entry's list position. Taken when the tile's depth range fits the word and no two entries share a depth (then
        // the word's order IS the (depth, id) order); every other tile is sorted below as before, from the same LDS list.
        constexpr int PB = SS_CAP <= 512 ? 9 : 10;
        static_assert(64 * EPL <= (1 << PB), "a list position fits the key's low bits");
        unsigned key[EPL];
        unsigned lmin = 0xffffffffu;
#pragma unroll
        for (int r = 0; r < EPL; ++r) {
          const int i = r * 64 + lane;
          const unsigned d = lds.depth[min(i, SS_CAP - 1)];
          key[r] = i < L ? d : 0xffffffffu;
          lmin = min(lmin, key[r]);
        }
        const unsigned dmin = wave_min_u32(lmin);
        bool bad = false;   // (max - min fits) == (every rel fits)
#pragma unroll
        for (int r = 0; r < EPL; ++r) {
          const int i = r * 64 + lane;
          bad |= i < L && !sortkey_fits(dmin, key[r], PB);
          key[r] = i < L ? sortkey_pack(key[r], dmin, (unsigned)i, PB) : SORTKEY_PAD;
        }
        if (__ballot(bad) == 0ull) {
          wave_bitonic_sort<EPL>(key, lane);
          // equal depths: neighbours in the sorted order -- inside the lane, and the next lane's first entry
          const unsigned next0 = (unsigned)__shfl_down((int)key[0], 1);
          bool tie = lane < 63 && !sortkey_is_padding(next0) && sortkey_same_depth(key[EPL - 1], next0, PB);
#pragma unroll
          for (int r = 0; r + 1 < EPL; ++r)
            tie |= !sortkey_is_padding(key[r + 1]) && sortkey_same_depth(key[r], key[r + 1], PB);
          if (__ballot(tie) == 0ull) {
            const unsigned s = (unsigned)bin_base + (unsigned)__builtin_amdgcn_readfirstlane((int)off);
            if (lane == 0) tile_range[t] = make_uint2(s, c);
            if (owns) {
              unsigned ids[EPL], pay[EPL];
#pragma unroll
              for (int r = 0; r < EPL; ++r) {
                const bool pad = sortkey_is_padding(key[r]);   // the padding's words are what the 64-bit sort leaves there
                const uint2 e = lds.idp[min(sortkey_pos(key[r], PB), (unsigned)SS_CAP - 1u)];
                ids[r] = pad ? 0xffffffffu : e.x;
                pay[r] = pad ? 0u : e.y;
              }
              store_list_entries<EPL>(sorted_id + s + lane * EPL, ids);
              store_list_entries<EPL>(sorted_dup + s + lane * EPL, pay);
            }
            return;
          }
        }
      }
      // ---- 64-bit key (depth bits << 32 | id) + payload
      if (lane == 0) atomicAdd(&line[8], 1u);   // tiles sorted on the 64-bit key (summed by list_stats)
      unsigned long long key[EPL];
      unsigned pay[EPL];
#pragma unroll
      for (int r = 0; r < EPL; ++r) {
        const int i = r * 64 + lane;
        const unsigned d = lds.depth[min(i, SS_CAP - 1)];
        const uint2 e = lds.idp[min(i, SS_CAP - 1)];
        key[r] = i < L ? (((unsigned long long)d << 32) | e.x) : ~0ull;
        pay[r] = i < L ? e.y : 0u;
      }
      wave_bitonic_sort<EPL>(key, pay, lane);
      const unsigned s = (unsigned)bin_base + (unsigned)__builtin_amdgcn_readfirstlane((int)off);
      if (lane == 0) tile_range[t] = make_uint2(s, c);
      if (owns) {
        unsigned ids[EPL];
#pragma unroll
        for (int r = 0; r < EPL; ++r) ids[r] = (unsigned)(key[r] & 0xffffffffull);
        store_list_entries<EPL>(sorted_id + s + lane * EPL, ids);
        store_list_entries<EPL>(sorted_dup + s + lane * EPL, pay);
      }
    };
    if (L <= 64) finish(std::integral_constant<int, 1>{});
    else if (L <= 128) finish(std::integral_constant<int, 2>{});
    else if (L <= 256) finish(std::integral_constant<int, 4>{});
    else if (SS_CAP <= 512 || L <= 512) finish(std::integral_constant<int, 8>{});
    else if constexpr (SS_CAP > 512) finish(std::integral_constant<int, 16>{});
    return;
  }
  // ---- long list: unsorted 16-byte items for the long-list kernels, like fine_bin ------------------------------------
  const unsigned s = (unsigned)bin_base + (unsigned)__builtin_amdgcn_readfirstlane((int)off);
  if (lane == 0) {
    tile_range[t] = make_uint2(s, c);
    long_tiles[atomicAdd(&hdr[HDR_LONG_COUNT], 1ull)] = (unsigned)t;
  }
  unsigned done = 0;
  for (unsigned i0 = 0; i0 < n; i0 += 64u * R) {   // R loads of the wave in flight per round trip
    uint4 lt[R];
#pragma unroll
    for (int k = 0; k < R; ++k) lt[k] = slab[min(i0 + 64u * k + lane, n - 1u)];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const bool hit = i0 + 64u * k + lane < n && ((lt[k].w >> bit) & 1u);
      const unsigned long long b = __ballot(hit);
      const unsigned pos = done + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
      if (hit) items[s + pos] = make_uint4(lt[k].x, lt[k].y, lt[k].z + (unsigned)__popc(lt[k].w & below), 0u);
      done += (unsigned)__popcll(b);
    }
  }
}

// longest list of the frame = max over the bins' maxima (select_sort_kernel), and the list statistics for the next
// frame's plan (SfgsFrame.feedback). Run by the first workgroup of the (always launched) long-list kernel: 256 threads.
__device__ void list_stats(int NCB, uint32_t* __restrict__ coarse_count, unsigned long long* hdr,
                           unsigned long long* __restrict__ feedback) {
  __shared__ unsigned ls_part[4], ls_over[4], ls_wide[4];
  unsigned m = 0, over = 0, wide = 0;
  for (int i = threadIdx.x; i < NCB; i += 256) {
    m = max(m, coarse_count[(size_t)i * CC_STRIDE + 4]);
    over += coarse_count[(size_t)i * CC_STRIDE + 5];
    wide += coarse_count[(size_t)i * CC_STRIDE + 8];
    // (a plan is single-use, include/sfgs.h: the bins' slot cursors, their maxima and the header's long-list words are
    // only reset by the next plan's memset)
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    m = max(m, (unsigned)__shfl_xor((int)m, d));
    over += (unsigned)__shfl_xor((int)over, d);
    wide += (unsigned)__shfl_xor((int)wide, d);
  }
  if ((threadIdx.x & 63) == 0) { ls_part[threadIdx.x >> 6] = m; ls_over[threadIdx.x >> 6] = over; ls_wide[threadIdx.x >> 6] = wide; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long mx = max(max(ls_part[0], ls_part[1]), max(ls_part[2], ls_part[3]));
    hdr[HDR_MAX_LIST] = mx;
    hdr[HDR_SORT_WIDE] = (unsigned long long)ls_wide[0] + ls_wide[1] + ls_wide[2] + ls_wide[3];
    if (feedback) {
      feedback[FB_VALID] = 1ull;
      feedback[FB_LONG_TILES] = hdr[HDR_LONG_COUNT];
      feedback[FB_MAX_LIST] = mx;
      feedback[FB_OVER_512] = (unsigned long long)ls_over[0] + ls_over[1] + ls_over[2] + ls_over[3];
    }
  }
  __syncthreads();
}

// K4a': the same register network with EPL = 16 keys per lane for lists of 513..1024 entries (low-elevation views, dense
// frames). A kernel of its own: 99 VGPRs would otherwise cut the occupancy of the common short lists. One wave per tile,
// persistent over the device-side list of long tiles. (Longer lists: the bucketed sort of sort_tiles_long_kernel.)
template <int EPL>
__global__ void __launch_bounds__(256)
sort_tiles_reg_long_kernel(const uint32_t* __restrict__ long_tiles, const unsigned long long* __restrict__ hdr,
                           const uint2* __restrict__ tile_range, const uint4* __restrict__ items,
                           uint32_t* __restrict__ sorted_id, uint32_t* __restrict__ sorted_dup) {
  const unsigned n_long = (unsigned)hdr[HDR_LONG_COUNT];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  for (unsigned li = blockIdx.x * 4 + wave; li < n_long; li += gridDim.x * 4) {
    const uint2 tr = tile_range[long_tiles[li]];
    const int L = (int)tr.y;
    if (L > 32 * EPL && L <= 64 * EPL) sort_tile_in_registers<EPL>(tr.x, L, lane, items, sorted_id, sorted_dup);
  }
}

// K4b: per-tile sort of the lists the register network does not take (L > 512), by 64-bit key
// (depth bits << 32 | Gaussian id) == ascending (depth, Gaussian id), SURVEY A.3. One 256-thread workgroup per tile,
// persistent over the device-side list of long tiles; normalised bitonic network (every comparator sorts ascending,
// so the +inf padding stays at the tail and comparators reaching past the end of the list are no-ops).
//   L <= CAP : one pass in LDS (keys + payload, 48 KB: three workgroups per CU). Dense frames (16 M Gaussians at
//              1080p: every list ~1 800 long) run entirely through this path.
//   L  > CAP : hybrid -- every CAP-chunk is sorted in LDS, then for each larger network size only the exchanges
//              with stride >= CAP touch global memory (in place, on the tile's own segment of 16-byte items); the
//              strides below CAP of that size are again one LDS pass per chunk. Global accesses are agent-scope
//              relaxed (they bypass the per-CU L1, so the waves of the workgroup see each other's exchanges after
//              the barrier).
template <int CAP>
__global__ void __launch_bounds__(256, 3)   // three workgroups per CU: what the 52 KB of LDS allow
sort_tiles_long_kernel(int lo, const uint32_t* __restrict__ long_tiles, const unsigned long long* __restrict__ hdr,
                       const uint2* __restrict__ tile_range, uint4* items, uint32_t* __restrict__ sorted_id,
                       uint32_t* __restrict__ sorted_dup, int stats_bins, uint32_t* __restrict__ coarse_count,
                       unsigned long long* hdr_w, unsigned long long* __restrict__ feedback) {
  __shared__ unsigned long long k[CAP];
  __shared__ uint32_t pl[CAP];
  constexpr int NT = 256;
  // behind select_sort_kernel (stats_bins > 0): the frame's list statistics are final now
  if (stats_bins > 0 && blockIdx.x == 0) list_stats(stats_bins, coarse_count, hdr_w, feedback);
  const unsigned n_long = (unsigned)hdr[HDR_LONG_COUNT];
  const int tid = threadIdx.x;
  // ---- bucketed sort (lists of up to 2 CAP entries): O(n) partition by depth, then small register sorts ----------------
  // The list is split into 256 equal-width depth bins (LDS histogram, counting scatter); consecutive bins are grouped
  // into segments of at most SEG entries and every segment is sorted by ONE WAVE in registers on the full 64-bit key
  // (depth bits, id) -- the network of the short lists, no barriers, no LDS exchanges. Only the depth bits and the
  // entry's 16-bit position live in LDS (6 bytes per entry: the same 48 KB hold 2 CAP entries); ids and duplicate indices
  // are gathered from the tile's item segment when a segment is loaded. A bitonic network over 4 096 entries has 78
  // barrier-separated LDS steps, over 8 192 entries 23 of its 91 steps went through global memory; this needs three
  // barriers and log^2(512) = 45 register steps per segment. Falls back to the network when one bin alone exceeds SEG
  // (a list concentrated in < 0.4 % of its own depth range) or all depths are equal.
  constexpr int BK_BINS = 256, SEG = 512, BK_CAP = 2 * CAP;
  uint32_t* bk_depth = reinterpret_cast<uint32_t*>(k);          // [BK_CAP] depth bits, grouped by bin
  uint16_t* bk_pos = reinterpret_cast<uint16_t*>(pl);           // [BK_CAP] position in the tile's item segment
  __shared__ unsigned bk_hist[BK_BINS], bk_start[BK_BINS + 1], bk_red[2 * (NT / 64)];
  __shared__ unsigned short bk_seg_bin[BK_BINS + 1], bk_next[BK_BINS];   // first bin of every segment (+ end marker)
  static_assert(NT == BK_BINS, "one thread per depth bin");
  __shared__ unsigned bk_nseg, bk_fallback;
  // Two LDS layouts: lists of up to CAP entries keep (depth, id, duplicate index) in LDS -- the tile's items are read from
  // memory exactly once; lists of up to 2 CAP entries keep (depth, 16-bit position) and gather id / duplicate index from
  // the item segment when a segment is sorted (a second, scattered read of the items).
  uint32_t* bk_id = reinterpret_cast<uint32_t*>(k) + CAP;         // [CAP]  (narrow layout only)
  auto bucket_sort = [&](unsigned s, int L, auto wide_tag) -> bool {
    constexpr bool WIDE = decltype(wide_tag)::value;
    const int lane = tid & 63, wave = tid >> 6;
    // the thread's depths stay in registers for all three passes (min / max, histogram, scatter): read from memory in
    // every pass, each pass was a chain of dependent global-load latencies
    constexpr int PER = (WIDE ? BK_CAP : CAP) / NT;
    unsigned dreg[PER], idreg[WIDE ? 1 : PER], dupreg[WIDE ? 1 : PER];
    unsigned dmin = 0xffffffffu, dmax = 0u;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int i = tid + NT * r;
      // unconditional loads from a clamped index (entries beyond L are never used: every later pass tests i < L)
      if constexpr (WIDE) {
        dreg[r] = items[s + min(i, L - 1)].y;
      } else {
        const uint4 it = items[s + min(i, L - 1)];
        dreg[r] = it.y; idreg[r] = it.x; dupreg[r] = it.z;
      }
    }
#pragma unroll
    for (int r = 0; r < PER; ++r)
      if (tid + NT * r < L) { dmin = min(dmin, dreg[r]); dmax = max(dmax, dreg[r]); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { dmin = min(dmin, (unsigned)__shfl_xor((int)dmin, o)); dmax = max(dmax, (unsigned)__shfl_xor((int)dmax, o)); }
    if (lane == 0) { bk_red[wave] = dmin; bk_red[NT / 64 + wave] = dmax; }
    if (tid < BK_BINS) bk_hist[tid] = 0u;
    __syncthreads();
    dmin = min(min(bk_red[0], bk_red[1]), min(bk_red[2], bk_red[3]));
    dmax = max(max(bk_red[4], bk_red[5]), max(bk_red[6], bk_red[7]));
    if (dmin == dmax) return false;                               // uniform across the workgroup
    // view depths are positive floats: their bit patterns order like the values, and the float arithmetic below is
    // monotonic in the depth (subtract, scale, truncate)
    const float fmin = __uint_as_float(dmin), scale = 255.5f / (__uint_as_float(dmax) - fmin);
    auto bin_of = [&](unsigned d) { return min((unsigned)((__uint_as_float(d) - fmin) * scale), (unsigned)(BK_BINS - 1)); };
#pragma unroll
    for (int r = 0; r < PER; ++r)
      if (tid + NT * r < L) atomicAdd(&bk_hist[bin_of(dreg[r])], 1u);
    __syncthreads();
    if (wave == 0) {   // exclusive scan of the 256 counts (4 per lane), largest bin
      unsigned c[4], sum = 0, big = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) { c[q] = bk_hist[lane * 4 + q]; sum += c[q]; big = max(big, c[q]); }
      unsigned incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const unsigned t = (unsigned)__shfl_up((int)incl, o); if (lane >= o) incl += t; }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) big = max(big, (unsigned)__shfl_xor((int)big, o));
      unsigned run = incl - sum;
#pragma unroll
      for (int q = 0; q < 4; ++q) { bk_start[lane * 4 + q] = run; bk_hist[lane * 4 + q] = run; run += c[q]; }   // hist -> cursors
      if (lane == 63) bk_start[BK_BINS] = run;
      if (lane == 0) bk_fallback = big > (unsigned)SEG ? 1u : 0u;
    }
    __syncthreads();
    if (bk_fallback) return false;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int i = tid + NT * r;
      if (i < L) {
        const unsigned pos = atomicAdd(&bk_hist[bin_of(dreg[r])], 1u);
        bk_depth[pos] = dreg[r];
        if constexpr (WIDE) bk_pos[pos] = (uint16_t)i;
        else { bk_id[pos] = idreg[r]; pl[pos] = dupreg[r]; }
      }
    }
    // greedy grouping of consecutive bins into segments of at most SEG entries: every bin finds, by binary search on the
    // prefix sums, the first bin that no longer fits a segment starting at itself; one thread then hops along
    {
      const unsigned base = bk_start[tid];          // NT == BK_BINS threads
      int lo_b = tid + 1, hi_b = BK_BINS;           // largest e in (tid, 256] with bk_start[e] - base <= SEG
      while (lo_b < hi_b) {
        const int mid = (lo_b + hi_b + 1) >> 1;
        if (bk_start[mid] - base <= (unsigned)SEG) lo_b = mid; else hi_b = mid - 1;
      }
      bk_next[tid] = (unsigned short)lo_b;
    }
    __syncthreads();
    if (tid == 0) {
      unsigned ns = 0, bb = 0;
      while (bb < (unsigned)BK_BINS && bk_start[bb] < (unsigned)L) { bk_seg_bin[ns++] = (unsigned short)bb; bb = bk_next[bb]; }
      bk_seg_bin[ns] = (unsigned short)BK_BINS;
      bk_nseg = ns;
    }
    __syncthreads();
    const unsigned nseg = bk_nseg;
    for (unsigned g = wave; g < nseg; g += NT / 64) {
      // a segment ends where the next one begins (empty bins in between belong to nobody)
      const unsigned a = bk_start[bk_seg_bin[g]], e = bk_start[bk_seg_bin[g + 1]];
      const int n = (int)(e - a);
      auto run_seg = [&](auto epl_tag) {
        constexpr int E = decltype(epl_tag)::value;
        unsigned long long key[E];
        unsigned pay[E];
#pragma unroll
        for (int r = 0; r < E; ++r) {
          const int i = r * 64 + lane;
          key[r] = ~0ull; pay[r] = 0u;
          if (i < n) {
            if constexpr (WIDE) {
              const uint4 it = items[s + bk_pos[a + i]];
              key[r] = ((unsigned long long)bk_depth[a + i] << 32) | it.x;
              pay[r] = it.z;
            } else {
              key[r] = ((unsigned long long)bk_depth[a + i] << 32) | bk_id[a + i];
              pay[r] = pl[a + i];
            }
          }
        }
        wave_bitonic_sort<E>(key, pay, lane);
#pragma unroll
        for (int r = 0; r < E; ++r) {
          const int q = lane * E + r;
          if (q < n) { sorted_id[s + a + q] = (unsigned)(key[r] & 0xffffffffull); sorted_dup[s + a + q] = pay[r]; }
        }
      };
      if (n <= 64) run_seg(std::integral_constant<int, 1>{});
      else if (n <= 128) run_seg(std::integral_constant<int, 2>{});
      else if (n <= 256) run_seg(std::integral_constant<int, 4>{});
      else run_seg(std::integral_constant<int, 8>{});
    }
    return true;
  };

  // comparators (i, i ^ mask-ish) of one network step restricted to LDS-resident positions [0, m)
  auto lds_mirror = [&](int m, int size) {   // first step of `size`: i <-> block_end - 1 - offset
    const int half = size >> 1;
    for (int c = tid; c < (m >> 1); c += NT) {
      const int blk = c / half, o = c - blk * half;
      const int i = blk * size + o, j = blk * size + size - 1 - o;
      const unsigned long long a = k[i], b = k[j];
      if (a > b) { k[i] = b; k[j] = a; const uint32_t x = pl[i]; pl[i] = pl[j]; pl[j] = x; }
    }
    __syncthreads();
  };
  auto lds_strides = [&](int m, int first_stride) {  // strides first_stride, first_stride/2, ..., 1
    for (int stride = first_stride; stride >= 1; stride >>= 1) {
      for (int c = tid; c < (m >> 1); c += NT) {
        const int i = 2 * stride * (c / stride) + (c % stride), j = i + stride;
        const unsigned long long a = k[i], b = k[j];
        if (a > b) { k[i] = b; k[j] = a; const uint32_t x = pl[i]; pl[i] = pl[j]; pl[j] = x; }
      }
      __syncthreads();
    }
  };

  // full sort of the m (power of two, <= CAP) entries in LDS: the bitonic network, one barrier per step. Only the
  // bucketed sort's fallback and the chunks of lists beyond 2 CAP entries come here (a register presort of the four
  // 1 024-entry quarters used to save 55 of the 78 steps at m = 4096, for 127 VGPRs: with the bucketed sort in front it
  // would only cost the common path its occupancy).
  auto sort_lds = [&](int m) {
    for (int size = 2; size <= m; size <<= 1) { lds_mirror(m, size); lds_strides(m, size >> 2); }
  };

  for (unsigned li = blockIdx.x; li < n_long; li += gridDim.x) {  // uniform per workgroup
    const uint2 tr = tile_range[long_tiles[li]];
    const unsigned s = tr.x;
    const long long L = (long long)tr.y;
    if (L <= lo) continue;
    __syncthreads();
    if (L <= CAP ? bucket_sort(s, (int)L, std::false_type{}) : (L <= BK_CAP && bucket_sort(s, (int)L, std::true_type{}))) continue;
    __syncthreads();
    long long n = 1;
    while (n < L) n <<= 1;
    if (n <= CAP) {  // ---- whole list in LDS -------------------------------------------------------------------
      const int m = (int)n;
      for (int i = tid; i < m; i += NT) {
        unsigned long long key = ~0ull;
        uint32_t d = 0;
        if (i < L) { const uint4 it = items[s + i]; key = ((unsigned long long)it.y << 32) | it.x; d = it.z; }
        k[i] = key; pl[i] = d;
      }
      __syncthreads();
      sort_lds(m);
      for (int i = tid; i < L; i += NT) { sorted_id[s + i] = (unsigned)(k[i] & 0xffffffffull); sorted_dup[s + i] = pl[i]; }
      continue;
    }
    // ---- hybrid: item i of the tile = 64-bit words 2i (key: id | depth << 32) and 2i + 1 (dup) ---------------------
    unsigned long long* w = reinterpret_cast<unsigned long long*>(items + s);
    auto ld = [&](long long i) { return __hip_atomic_load(&w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto st = [&](long long i, unsigned long long v) { __hip_atomic_store(&w[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto chunk_load = [&](long long base) {
      for (int i = tid; i < CAP; i += NT) {
        unsigned long long key = ~0ull;
        uint32_t d = 0;
        if (base + i < L) { key = ld(2 * (base + i)); d = (uint32_t)ld(2 * (base + i) + 1); }
        k[i] = key; pl[i] = d;
      }
      __syncthreads();
    };
    auto chunk_store = [&](long long base) {
      for (int i = tid; i < CAP; i += NT)
        if (base + i < L) { st(2 * (base + i), k[i]); st(2 * (base + i) + 1, (unsigned long long)pl[i]); }
      __syncthreads();
    };
    auto global_cmpx = [&](long long i, long long j) {
      if (j >= L) return;  // +inf padding never moves down
      const unsigned long long a = ld(2 * i), b = ld(2 * j);
      if (a > b) {
        const unsigned long long pa = ld(2 * i + 1), pb = ld(2 * j + 1);
        st(2 * i, b); st(2 * j, a); st(2 * i + 1, pb); st(2 * j + 1, pa);
      }
    };
    for (long long base = 0; base < L; base += CAP) {  // every chunk fully sorted (network sizes 2 .. CAP)
      chunk_load(base);
      sort_lds(CAP);
      chunk_store(base);
    }
    for (long long size = 2 * (long long)CAP; size <= n; size <<= 1) {
      const long long half = size >> 1;
      for (long long c = tid; c < (n >> 1); c += NT) {  // mirror step of this size: always crosses chunks
        const long long blk = c / half, o = c - blk * half;
        global_cmpx(blk * size + o, blk * size + size - 1 - o);
      }
      __syncthreads();
      for (long long stride = half >> 1; stride >= CAP; stride >>= 1) {
        for (long long c = tid; c < (n >> 1); c += NT) global_cmpx(2 * stride * (c / stride) + (c % stride),
                                                                      2 * stride * (c / stride) + (c % stride) + stride);
        __syncthreads();
      }
      for (long long base = 0; base < L; base += CAP) {  // strides CAP/2 .. 1 stay inside a chunk
        chunk_load(base);
        lds_strides(CAP, CAP >> 1);
        chunk_store(base);
      }
    }
    for (long long i = tid; i < L; i += NT) {
      sorted_id[s + i] = (unsigned)(ld(2 * i) & 0xffffffffull);
      sorted_dup[s + i] = (unsigned)(ld(2 * i + 1) & 0xffffffffull);
    }
  }
}

// Route of the render stage's fine binning + short-list sort: the "sort" option (sfgs_set_option) forces one (tests, A/B
// runs); otherwise the caller's SHORT_LISTS hint picks the fused kernel. Both routes build bit-identical lists.
// Returns 0 (split), 512 or 1024 (the fused kernel's list capacity: "fused1024" / the MEDIUM_LISTS hint).
static int sort_fused(uint32_t launch_hints) {
  switch (option(OPT_SORT)) {
    case SORT_SPLIT: return 0;
    case SORT_FUSED: return 512;
    case SORT_FUSED1024: return 1024;
    case SORT_FUSED768: return 768;
    default: break;
  }
  if (launch_hints & SFGS_HINT_MEDIUM_LISTS) return (launch_hints & SFGS_HINT_LISTS_768) ? 768 : 1024;
  return (launch_hints & SFGS_HINT_SHORT_LISTS) ? 512 : 0;
}

constexpr int SORT_CAP = 4096;

int sort_tile_lists(const SfgsFrame* frame, const TilesView& tv, const BinsView& bv, int64_t dup_capacity,
                    int64_t coarse_capacity, int64_t num_duplicates, hipStream_t stream) {
  const int W = frame->image_width, H = frame->image_height;
  const int64_t NCB = coarse_bins(W, H);
  const int TX8 = tiles8_x(W), TY8 = tiles8_y(H), T8 = TX8 * TY8, CX = coarse_x(W);
  // Two routes to the sorted per-tile lists (bit-identical results): select_sort_kernel (no per-tile items in memory, one
  // launch less: faster for lists of a few hundred entries and bins of a few thousand items -- the caller's SHORT_LISTS
  // hint) or fine_bin + the sort kernels with the items in memory between them (long lists, crowded bins)
  const int fused_cap = sort_fused(frame->launch_hints);
  const bool fused = fused_cap != 0;
  if (fused) {
    // option "sort_key": the short lists' sort on one exact 32-bit word per entry wherever a tile allows it ("narrow"), or on
    // the 64-bit key everywhere ("wide"); bit-identical lists either way. "auto" = narrow for the 512-entry form only: the
    // low-elevation regime (lists of 513 .. 652 entries, 768 / 1 024 forms) lost 0.8 % with it, presumably to tiles that pass the
    // range test, show two equal depths and are sorted twice (profiles/r12_select_sort_narrow_key_ab.txt)
    const int narrow = option(OPT_SORT_KEY) == SORT_KEY_NARROW || (option(OPT_SORT_KEY) == SORT_KEY_AUTO && fused_cap <= 512);
    { ProfScope ps_(KID_SORT_SMALL, stream);
      if (fused_cap > 768)
        hipLaunchKernelGGL(select_sort_kernel<1024>, dim3((unsigned)NCB * COARSE), dim3(256), 0, stream, TX8, TY8, CX,
                           (int)NCB, tv.coarse_count, bv.csr, bv.slabs, (unsigned)coarse_capacity,
                           (unsigned long long)dup_capacity, tv.tile_range, bv.items, tv.long_tiles, tv.hdr, bv.sorted_id,
                           bv.sorted_dup, narrow);
      else if (fused_cap > 512)   // 36 KB of LDS per workgroup: four workgroups per CU instead of three
        hipLaunchKernelGGL(select_sort_kernel<768>, dim3((unsigned)NCB * COARSE), dim3(256), 0, stream, TX8, TY8, CX,
                           (int)NCB, tv.coarse_count, bv.csr, bv.slabs, (unsigned)coarse_capacity,
                           (unsigned long long)dup_capacity, tv.tile_range, bv.items, tv.long_tiles, tv.hdr, bv.sorted_id,
                           bv.sorted_dup, narrow);
      else
        hipLaunchKernelGGL(select_sort_kernel<512>, dim3((unsigned)NCB * COARSE), dim3(256), 0, stream, TX8, TY8, CX,
                           (int)NCB, tv.coarse_count, bv.csr, bv.slabs, (unsigned)coarse_capacity,
                           (unsigned long long)dup_capacity, tv.tile_range, bv.items, tv.long_tiles, tv.hdr, bv.sorted_id,
                           bv.sorted_dup, narrow); }
    SFGS_POST_LAUNCH("select_sort", stream, frame->debug);
  } else {
    { ProfScope ps_(KID_FINE_BIN, stream);
      hipLaunchKernelGGL(fine_bin_kernel, dim3((unsigned)NCB), dim3(256), 0, stream, TX8, TY8, CX, (int)NCB,
                         tv.coarse_count, bv.csr, bv.slabs, (unsigned)coarse_capacity, (unsigned long long)dup_capacity,
                         tv.tile_range, bv.items, tv.long_tiles, tv.hdr); }
    SFGS_POST_LAUNCH("fine_bin", stream, frame->debug);
  }
  if (num_duplicates != 0) {  // < 0: unknown (render enqueued before the counters were read)
    if (!fused) {
      { ProfScope ps_(KID_SORT_SMALL, stream);
        hipLaunchKernelGGL(sort_tiles_reg_kernel, dim3((T8 + 3) / 4), dim3(256), 0, stream, T8, tv.tile_range, bv.items,
                           bv.sorted_id, bv.sorted_dup, (const unsigned long long*)tv.hdr,
                           (unsigned long long*)frame->feedback); }
      SFGS_POST_LAUNCH("sort_tiles_small", stream, frame->debug);
    }
    const int stats_bins = fused ? (int)NCB : 0;
    if (frame->launch_hints & SFGS_HINT_FEW_LONG_LISTS) {
      // the caller expects (next to) no list beyond 512 entries: ONE catch-all launch -- the LDS kernel takes every long
      // list, whatever its size class -- instead of three that each cost ~5 us of queue time when they find nothing
      ProfScope ps_(KID_SORT_LDS, stream);
      hipLaunchKernelGGL(sort_tiles_long_kernel<SORT_CAP>, dim3(std::min(T8, 768)), dim3(256), 0, stream, REG_SORT_SMALL,
                         tv.long_tiles, tv.hdr, tv.tile_range, bv.items, bv.sorted_id, bv.sorted_dup, stats_bins,
                         tv.coarse_count, tv.hdr, (unsigned long long*)frame->feedback);
    } else {
    // size classes: 513..1024 -> register network with 16 keys per lane; longer -> bucketed sort (a 32-key register
    // network used to take 1025..2048: 195 VGPRs, one more launch, and slower than the buckets -- city 0.179 -> 0.152 ms)
    { ProfScope ps_(KID_SORT_REG_LONG, stream);
      hipLaunchKernelGGL(sort_tiles_reg_long_kernel<16>, dim3(std::min((T8 + 3) / 4, 2048)), dim3(256), 0, stream,
                         tv.long_tiles, tv.hdr, tv.tile_range, bv.items, bv.sorted_id, bv.sorted_dup); }
    SFGS_POST_LAUNCH("sort_tiles_reg_long", stream, frame->debug);
    { ProfScope ps_(KID_SORT_LDS, stream);
      hipLaunchKernelGGL(sort_tiles_long_kernel<SORT_CAP>, dim3(std::min(T8, 768)), dim3(256), 0, stream, REG_SORT_MAX,
                         tv.long_tiles, tv.hdr, tv.tile_range, bv.items, bv.sorted_id, bv.sorted_dup, stats_bins,
                         tv.coarse_count, tv.hdr, (unsigned long long*)frame->feedback); }
    }
    SFGS_POST_LAUNCH("sort_tiles_long", stream, frame->debug);
  }
  return SFGS_OK;
}

}  // namespace sfgs
