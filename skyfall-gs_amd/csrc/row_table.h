// row_table.h -- the multi-tensor row walk of the two model-editing gathers (compact.hip: compact_gather_kernel, densify.hip:
// densify_gather_kernel), once: ONE launch moves the rows of many tensors. A table in the kernel arguments gives every tensor a run
// of workgroups; a workgroup of RT_NT threads owns RT_WORD_CHUNK consecutive units (4-byte words, or bytes) of its tensor, a thread
// RT_WORDS_PER_THREAD of them at stride RT_NT. What a kernel does with a unit's row and column is its own.
#pragma once
#include "sfgs_internal.h"

namespace sfgs {

constexpr int RT_NT = 256, RT_WORDS_PER_THREAD = 8, RT_WORD_CHUNK = RT_NT * RT_WORDS_PER_THREAD;

template <int CAP>
struct RowTable {
  const void* src[CAP];
  void* dst[CAP];
  unsigned row_units[CAP];   // row size in units
  unsigned block_end[CAP];   // the tensor's workgroups end here (exclusive, running)
  int count;
};

struct RowWalk {
  int ti;                    // the workgroup's tensor
  unsigned ru;               // its row size in units
  const void* src;           // its rows, and where they go
  void* dst;
  long long base, words;     // the workgroup's first unit; the tensor's units, N * ru
};

// The workgroup's tensor and, per unit k of the thread, its row -- clamped to N - 1, so that a load through it needs no
// predicate --, its column and the row's byte of row_byte[N] (the keep flag, the decision code): the first of a gather's three
// phases of loads. Unit k is base + threadIdx.x + k * RT_NT; it exists only when that is < words.
template <int CAP>
__device__ __forceinline__ RowWalk row_table_walk(const RowTable<CAP>& tab, long long N, const unsigned char* __restrict__ row_byte,
                                                  long long (&rowv)[RT_WORDS_PER_THREAD], unsigned (&colv)[RT_WORDS_PER_THREAD],
                                                  unsigned char (&bytev)[RT_WORDS_PER_THREAD]) {
  RowWalk w;
  w.ti = 0;
  while (w.ti + 1 < tab.count && blockIdx.x >= tab.block_end[w.ti]) ++w.ti;
  const unsigned first = w.ti ? tab.block_end[w.ti - 1] : 0u;
  w.ru = tab.row_units[w.ti];
  const unsigned ru = w.ru;
  w.src = tab.src[w.ti]; w.dst = tab.dst[w.ti];
  w.words = N * (long long)ru;
  w.base = (long long)(blockIdx.x - first) * RT_WORD_CHUNK;   // block-uniform
  const long long row0 = w.base / ru;                         // one 64-bit division per block
  const unsigned rem0 = (unsigned)(w.base - row0 * ru);
  const float inv = 1.0f / (float)ru;
#pragma unroll
  for (int k = 0; k < RT_WORDS_PER_THREAD; ++k) {
    // (rem0 + off) / ru with x < 2^24 (ru < 2^22, off < 2^11): float estimate + one correction step is exact
    const unsigned x = rem0 + threadIdx.x + k * RT_NT;
    unsigned q = (unsigned)((float)x * inv);
    if (q * ru > x) --q; else if ((q + 1) * ru <= x) ++q;
    rowv[k] = min(row0 + (long long)q, N - 1);
    colv[k] = x - q * ru;
    bytev[k] = row_byte[rowv[k]];
  }
  return w;
}

// Host: the next table from tensors[first ...] (TensorT: src, dst, row_bytes -- checked by the caller, row_bytes a multiple of
// `unit` and < 2^22). Tensors with empty rows are skipped; the table closes at CAP tensors or before the launch's grid would
// reach 2^31 workgroups. *blocks = the grid (0: only empty tensors were left), *next = where the following table starts; the
// table's entries are the non-empty tensors of [first, *next) in order.
template <int CAP, typename TensorT>
int row_table_pack(const TensorT* tensors, int count, int first, long long N, int unit, RowTable<CAP>* tab, uint64_t* blocks,
                   int* next) {
  tab->count = 0;
  *blocks = 0;
  int i = first;
  for (; i < count && tab->count < CAP; ++i) {
    if (tensors[i].row_bytes == 0) continue;
    const uint64_t ru = (uint64_t)tensors[i].row_bytes / unit;
    const uint64_t nb = ((uint64_t)N * ru + RT_WORD_CHUNK - 1) / RT_WORD_CHUNK;
    SFGS_REQUIRE(nb < (1ull << 31), SFGS_E_UNSUPPORTED, "tensor %d: too large for one launch", i);
    if (*blocks + nb >= (1ull << 31)) break;
    *blocks += nb;
    tab->src[tab->count] = tensors[i].src; tab->dst[tab->count] = tensors[i].dst;
    tab->row_units[tab->count] = (unsigned)ru; tab->block_end[tab->count] = (unsigned)*blocks;
    ++tab->count;
  }
  *next = i;
  return SFGS_OK;
}

}  // namespace sfgs
