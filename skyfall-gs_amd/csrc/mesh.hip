// mesh.hip -- the triangle soup of tsdf.hip finished on the device: welded into an indexed mesh, its connected components
// labelled and counted, small components / degenerate faces removed. Everything is integers and copied bytes; include/sfgs.h states
// the results in words, tests/mesh_np.py in numpy, and this file is held to that restatement byte for byte. mesh_math.h has what
// is decided per element (key, hash, face rules), built for the host too by tests/host_check/mesh_check.cpp.
//   WELD (sfgs_mesh_weld), q = 3 t + c the flat soup vertex index, Q = 3 n:
//     1. weld_insert_kernel  a thread per q: open addressing over 32-bit slots that hold soup vertex indices (MESH_EMPTY = none),
//        linear probing from mesh_hash(key). Empty slot: compare-and-swap q in. Occupied by p: compare the soup's words at p and q
//        (the soup is read-only, so whatever index a slot ever held witnesses the slot's key); equal -> fetch_min(slot, q), done;
//        else the next slot. The thread remembers its slot. After the kernel a key's slot holds rep = the key's smallest q.
//     2. weld_rep_kernel     rep_of[q] = table[slot_of[q]] (in place), flag[q] = (rep_of[q] == q).
//     3. the row compaction of compact.hip on the flags: its plan ranks the representatives in order of first appearance
//        (vid = the exclusive rank), its gather writes V[vid] = S[rep] and colour[vid] = C[rep].
//     4. weld_faces_kernel   F[q] = rank[rep_of[q]]; the count goes into the state.
//   COMPONENTS (sfgs_mesh_components): lock-free union-find, parents only ever decrease, so a chain ends at its component's minimum.
//     1. cc_init_kernel      parent[v] = v.
//     2. cc_hook_kernel      a thread per face, edges (a, b) and (b, c) ((c, a) joins nothing new): find both roots, hook the
//        larger under the smaller by compare-and-swap on parent[hi] == hi, on failure go on from what the swap returned.
//        Finds halve their path with fetch_min (an ancestor is smaller than the parent it replaces).
//     3. cc_label_kernel     label[v] = the root of v's chain (the kernel boundary made every hook visible; plain loads);
//        vertices_in[label] += 1 and the number of roots, summed per wave and per workgroup before any atomic.
//     4. cc_faces_kernel     triangles[label[F[t][0]]] += 1, the same way.
//   CLEAN (sfgs_mesh_clean): clean_mark_kernel writes the keep bytes of faces and vertices from the caller's per-root keep bytes,
//     compact.hip ranks both and moves the vertex rows, clean_faces_kernel moves the kept faces through the vertex ranks.
// Shared mutable tables (the slots, parent) are read and written, inside the kernels that mutate them, with agent-scope relaxed
// atomics only. Every probe, find and retry loop has a trip bound that valid input cannot reach (the slot count, m, MESH_CAS_RETRIES);
// reaching it sets a status bit and leaves the loop. Every index read from a face is checked against m before it is used (a bad
// one sets MESH_ST_BAD_INDEX and the face is skipped); a slot's content is a soup index < Q by construction, checked all the same.
// Integer atomics only; no float atomics, no LDS beyond the per-workgroup sums, no kernel waits for another workgroup.
// No profiler ids of its own (the compaction keeps its two).
#include "sfgs_internal.h"
#include "mesh_math.h"

namespace sfgs {

constexpr int MESH_THREADS = 256;
constexpr int MESH_WAVES = MESH_THREADS / 64;

#define MESH_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ void mesh_raise(long long* __restrict__ state, unsigned bits) {
  if (bits) __hip_atomic_fetch_or((unsigned long long*)&state[2], (unsigned long long)bits, MESH_RLX);
}

// ---- weld ------------------------------------------------------------------------------------------------------------------------
template <bool STATS>
__global__ void __launch_bounds__(MESH_THREADS)
weld_insert_kernel(const uint32_t* __restrict__ soup, long long Q, uint32_t* table, unsigned long long slots,
                   uint32_t* __restrict__ slot_of, long long* __restrict__ state) {
  const long long q = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  unsigned long long probes = 0;
  if (q < Q) {
    const uint32_t mask = (uint32_t)(slots - 1);
    const MeshKey key = mesh_key(soup, q);
    uint32_t s = mesh_hash(key) & mask;
    bool done = false;
    unsigned long long trip = 0;
    for (; trip < slots; ++trip) {
      uint32_t cur = __hip_atomic_load(&table[s], MESH_RLX);
      if (cur == MESH_EMPTY) {
        uint32_t expected = MESH_EMPTY;
        if (__hip_atomic_compare_exchange_strong(&table[s], &expected, (uint32_t)q, __ATOMIC_RELAXED, MESH_RLX)) { done = true; break; }
        cur = expected;                                  // somebody's index went in first: it witnesses the slot's key
      }
      if ((long long)cur < Q && mesh_key_equal(mesh_key(soup, (long long)cur), key)) {
        if ((uint32_t)q < cur) __hip_atomic_fetch_min(&table[s], (uint32_t)q, MESH_RLX);
        done = true;
        break;
      }
      s = (s + 1u) & mask;
    }
    if (!done) mesh_raise(state, MESH_ST_PROBE_BOUND);
    slot_of[q] = s;                                      // < slots either way
    probes = trip + 1;
  }
  if (STATS) {                                           // diagnostics (tools/bench_mesh.py): slots looked at, summed per wave
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) probes += __shfl_down(probes, d);
    if (lane_id() == 0 && probes) __hip_atomic_fetch_add((unsigned long long*)&state[3], probes, MESH_RLX);
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
weld_rep_kernel(const uint32_t* __restrict__ table, uint32_t* __restrict__ slot_rep, unsigned char* __restrict__ flag, long long Q) {
  const long long q = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (q >= Q) return;
  uint32_t rep = table[slot_rep[q]];
  if ((long long)rep >= Q) rep = (uint32_t)q;            // only after a probe bound (flagged): stay in range
  slot_rep[q] = rep;
  flag[q] = rep == (uint32_t)q ? 1 : 0;
}

__global__ void __launch_bounds__(MESH_THREADS)
weld_faces_kernel(const uint32_t* __restrict__ rep_of, const uint32_t* __restrict__ rank, int32_t* __restrict__ faces, long long Q) {
  const long long q = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (q >= Q) return;
  faces[q] = (int32_t)rank[rep_of[q]];                  // rep_of[q] < Q: weld_rep_kernel
}

// state[0] = a ? *a : av, state[1] = b ? *b : bv (one thread)
__global__ void mesh_sizes_kernel(long long* __restrict__ state, const unsigned long long* __restrict__ a, long long av,
                                  const unsigned long long* __restrict__ b, long long bv) {
  state[0] = a ? (long long)*a : av;
  state[1] = b ? (long long)*b : bv;
}

// ---- counting into few words -----------------------------------------------------------------------------------------------------
// arr[label] += 1 for every active thread, every thread of the workgroup calling. The lanes of a wave that share a label add once;
// a wave whose lanes all share one label hands its sum to the workgroup, where neighbouring waves with the same label add once.
template <int NT>
__device__ __forceinline__ void mesh_count_add(int32_t* __restrict__ arr, int label, bool active, int* sm_label, int* sm_count) {
  const unsigned lane = lane_id(), wave = threadIdx.x >> 6;
  const unsigned long long all = __ballot(active);
  int uni_label = -1, uni_count = 0;
  if (all) {                                             // wave-uniform
    const int l0 = __shfl(label, __ffsll((long long)all) - 1);
    const unsigned long long same = __ballot(active && label == l0);
    if (same == all) {
      uni_label = l0;
      uni_count = __popcll(same);
    } else {
      unsigned long long todo = all;
      while (todo) {                                     // one round per distinct label of the wave
        const int lead = __ffsll((long long)todo) - 1;
        const int lb = __shfl(label, lead);
        const unsigned long long grp = __ballot(active && label == lb) & todo;
        if ((int)lane == lead) __hip_atomic_fetch_add(&arr[lb], (int32_t)__popcll(grp), MESH_RLX);
        todo &= ~grp;
      }
    }
  }
  if (lane == 0) { sm_label[wave] = uni_label; sm_count[wave] = uni_count; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int cur = -1, cnt = 0;
    for (int w = 0; w < NT / 64; ++w) {
      if (sm_label[w] != cur) {
        if (cur >= 0 && cnt) __hip_atomic_fetch_add(&arr[cur], cnt, MESH_RLX);
        cur = sm_label[w];
        cnt = 0;
      }
      cnt += sm_count[w];
    }
    if (cur >= 0 && cnt) __hip_atomic_fetch_add(&arr[cur], cnt, MESH_RLX);
  }
  __syncthreads();
}

// ---- components ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS) cc_init_kernel(int32_t* __restrict__ parent, long long m) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v < m) parent[v] = (int32_t)v;
}

// the root of v's chain, halving the path on the way; -1 when the chain is longer than m (it cannot be)
__device__ __forceinline__ int cc_find(int32_t* parent, int v, long long m, unsigned* status) {
  int x = v;
  for (long long trip = 0; trip <= m; ++trip) {
    const int p = __hip_atomic_load(&parent[x], MESH_RLX);
    if (p == x) return x;
    const int gp = __hip_atomic_load(&parent[p], MESH_RLX);
    if (gp == p) return p;
    __hip_atomic_fetch_min(&parent[x], gp, MESH_RLX);    // gp < p: an ancestor further up
    x = gp;
  }
  *status |= MESH_ST_FIND_BOUND;
  return -1;
}

__device__ __forceinline__ void cc_unite(int32_t* parent, int u, int v, long long m, unsigned* status) {
  if (u == v) return;
  int ru = cc_find(parent, u, m, status), rv = cc_find(parent, v, m, status);
  for (int tries = 0; tries < MESH_CAS_RETRIES; ++tries) {
    if (ru < 0 || rv < 0 || ru == rv) return;
    const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    int expected = hi;
    if (__hip_atomic_compare_exchange_strong(&parent[hi], &expected, lo, __ATOMIC_RELAXED, MESH_RLX)) return;
    ru = cc_find(parent, expected, m, status);           // hi was hooked meanwhile, under `expected` < hi
    rv = cc_find(parent, lo, m, status);
  }
  *status |= MESH_ST_CAS_BOUND;
}

__global__ void __launch_bounds__(MESH_THREADS)
cc_hook_kernel(const int32_t* __restrict__ faces, long long n, long long m, int32_t* parent, long long* __restrict__ state) {
  const long long t = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (t >= n) return;                                    // no barrier follows
  const int a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
  unsigned status = 0;
  if (mesh_index_ok(a, m) && mesh_index_ok(b, m) && mesh_index_ok(c, m)) {
    cc_unite(parent, a, b, m, &status);
    cc_unite(parent, b, c, m, &status);
  } else {
    status = MESH_ST_BAD_INDEX;
  }
  mesh_raise(state, status);
}

__global__ void __launch_bounds__(MESH_THREADS)
cc_label_kernel(const int32_t* __restrict__ parent, long long m, int32_t* __restrict__ labels, int32_t* __restrict__ vertices_in,
                long long* __restrict__ state) {
  __shared__ int sm_label[MESH_WAVES], sm_count[MESH_WAVES];
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  const bool active = v < m;
  int root = 0;
  unsigned status = 0;
  if (active) {
    int x = (int)v;
    long long trip = 0;
    for (; trip <= m; ++trip) {
      const int p = parent[x];
      if (p == x || !mesh_index_ok(p, m)) break;
      x = p;
    }
    if (trip > m) status = MESH_ST_FIND_BOUND;
    root = x;
    labels[v] = root;
  }
  mesh_raise(state, status);
  mesh_count_add<MESH_THREADS>(vertices_in, root, active, sm_label, sm_count);
  const int roots = __syncthreads_count(active && root == (int)v);
  if (threadIdx.x == 0 && roots) __hip_atomic_fetch_add((unsigned long long*)&state[0], (unsigned long long)roots, MESH_RLX);
}

__global__ void __launch_bounds__(MESH_THREADS)
cc_faces_kernel(const int32_t* __restrict__ faces, long long n, long long m, const int32_t* __restrict__ labels,
                int32_t* __restrict__ triangles) {
  __shared__ int sm_label[MESH_WAVES], sm_count[MESH_WAVES];
  const long long t = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  bool active = false;
  int root = 0;
  if (t < n) {
    const int a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
    if (mesh_index_ok(a, m) && mesh_index_ok(b, m) && mesh_index_ok(c, m)) {      // a bad face was flagged by cc_hook_kernel
      root = labels[a];
      active = mesh_index_ok(root, m);
    }
  }
  mesh_count_add<MESH_THREADS>(triangles, root, active, sm_label, sm_count);
}

__global__ void __launch_bounds__(MESH_THREADS)
mesh_vet_kernel(const int32_t* __restrict__ faces, long long n, long long m, long long* __restrict__ state) {
  const long long t = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (t >= n) return;
  const bool ok = mesh_index_ok(faces[3 * t], m) && mesh_index_ok(faces[3 * t + 1], m) && mesh_index_ok(faces[3 * t + 2], m);
  if (!ok) mesh_raise(state, MESH_ST_BAD_INDEX);
}

// ---- clean -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS)
clean_mark_kernel(const int32_t* __restrict__ faces, long long n, long long m, const int32_t* __restrict__ labels,
                  const unsigned char* __restrict__ keep_root, int drop_degenerate, unsigned char* __restrict__ keep_face,
                  unsigned char* __restrict__ keep_vertex, long long* __restrict__ state) {
  const long long t = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (t >= n) return;
  const int a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
  bool keep = false;
  if (mesh_index_ok(a, m) && mesh_index_ok(b, m) && mesh_index_ok(c, m)) {
    const int root = labels[a];
    if (mesh_index_ok(root, m)) keep = keep_root[root] != 0 && !(drop_degenerate && mesh_face_degenerate(a, b, c));
    else mesh_raise(state, MESH_ST_BAD_INDEX);
  } else {
    mesh_raise(state, MESH_ST_BAD_INDEX);
  }
  keep_face[t] = keep ? 1 : 0;
  if (keep) { keep_vertex[a] = 1; keep_vertex[b] = 1; keep_vertex[c] = 1; }      // every writer stores the same byte
}

__global__ void __launch_bounds__(MESH_THREADS)
clean_faces_kernel(const int32_t* __restrict__ faces, long long n, const unsigned char* __restrict__ keep_face,
                   const uint32_t* __restrict__ face_rank, const uint32_t* __restrict__ vertex_rank, int32_t* __restrict__ out) {
  const long long t = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (t >= n || !keep_face[t]) return;                   // a kept face has its three indices in range: clean_mark_kernel
  const long long r = face_rank[t];
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * r + c] = (int32_t)vertex_rank[faces[3 * t + c]];
}

}  // namespace sfgs

using namespace sfgs;

namespace {

inline unsigned mesh_blocks(long long items) { return (unsigned)((items + MESH_THREADS - 1) / MESH_THREADS); }

struct WeldScratch {
  uint32_t* table;          // [slots]
  uint32_t* slot_rep;       // [Q] the thread's slot, then its key's representative
  unsigned char* flag;      // [Q]
  void* compact;            // cp_scratch_bytes(Q)
  size_t compact_bytes, total;
};
WeldScratch weld_view(void* base, long long n) {
  const long long Q = 3 * n;
  const size_t slots = (size_t)mesh_weld_slots(n);
  WeldScratch w;
  char* p = (char*)base;
  size_t off = 0;
  w.table = (uint32_t*)(p + off); off += align_up(slots * 4, 256);
  w.slot_rep = (uint32_t*)(p + off); off += align_up((size_t)Q * 4, 256);
  w.flag = (unsigned char*)(p + off); off += align_up((size_t)Q, 256);
  w.compact = p + off; w.compact_bytes = cp_scratch_bytes(Q); off += w.compact_bytes;
  w.total = off;
  return w;
}

struct CleanScratch {
  unsigned char *keep_vertex, *keep_face;
  void *plan_vertex, *plan_face;
  size_t plan_vertex_bytes, plan_face_bytes, total;
};
CleanScratch clean_view(void* base, long long m, long long n) {
  CleanScratch c;
  char* p = (char*)base;
  size_t off = 0;
  c.keep_vertex = (unsigned char*)(p + off); off += align_up((size_t)m + 1, 256);
  c.keep_face = (unsigned char*)(p + off); off += align_up((size_t)n + 1, 256);
  c.plan_vertex = p + off; c.plan_vertex_bytes = cp_scratch_bytes(m); off += c.plan_vertex_bytes;
  c.plan_face = p + off; c.plan_face_bytes = cp_scratch_bytes(n); off += c.plan_face_bytes;
  c.total = off;
  return c;
}

int mesh_check_sizes(const char* what, int64_t m, int64_t n) {
  SFGS_REQUIRE(m >= 0 && m <= MESH_MAX_VERTICES, SFGS_E_ARG, "%s: %lld vertices, 0 ... 2^31 - 1", what, (long long)m);
  SFGS_REQUIRE(n >= 0 && n <= MESH_MAX_TRIANGLES, SFGS_E_ARG, "%s: %lld triangles, 0 ... 2^29", what, (long long)n);
  return SFGS_OK;
}

}  // namespace

extern "C" size_t sfgs_mesh_weld_scratch_bytes(int64_t n) {
  if (n < 0 || n > MESH_MAX_TRIANGLES) {
    sfgs::set_error("sfgs_mesh_weld_scratch_bytes: %lld triangles, 0 ... 2^29", (long long)n);
    return 0;
  }
  return weld_view(nullptr, n).total;
}

extern "C" int sfgs_mesh_weld(const float* soup, const float* soup_colors, int64_t n, float* vertices, float* colors, int32_t* faces,
                              long long* state, int32_t flags, void* scratch, size_t scratch_bytes, void* stream_) {
  if (const int rc = mesh_check_sizes("sfgs_mesh_weld", 0, n)) return rc;
  SFGS_REQUIRE(state, SFGS_E_ARG, "sfgs_mesh_weld: NULL state");
  SFGS_REQUIRE((flags & ~1) == 0, SFGS_E_ARG, "sfgs_mesh_weld: flags %d", flags);
  SFGS_REQUIRE((soup_colors == nullptr) == (colors == nullptr), SFGS_E_ARG, "sfgs_mesh_weld: soup_colors and colors come together");
  hipStream_t stream = (hipStream_t)stream_;
  if (n == 0) {                                          // m = 0, and no launch that indexes anything
    SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
    return SFGS_OK;
  }
  SFGS_REQUIRE(soup && vertices && faces && scratch, SFGS_E_ARG, "sfgs_mesh_weld: NULL argument");
  const WeldScratch w = weld_view(scratch, n);
  SFGS_REQUIRE(scratch_bytes >= w.total, SFGS_E_ARG, "mesh weld scratch too small: %zu < %zu", scratch_bytes, w.total);
  const long long Q = 3 * (long long)n;
  const unsigned long long slots = mesh_weld_slots(n);
  SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
  SFGS_CHECK_HIP(hipMemsetAsync(w.table, 0xff, (size_t)slots * 4, stream));
  const dim3 grid(mesh_blocks(Q)), block(MESH_THREADS);
  if (flags & 1)
    hipLaunchKernelGGL(weld_insert_kernel<true>, grid, block, 0, stream, (const uint32_t*)soup, Q, w.table, slots, w.slot_rep, state);
  else
    hipLaunchKernelGGL(weld_insert_kernel<false>, grid, block, 0, stream, (const uint32_t*)soup, Q, w.table, slots, w.slot_rep, state);
  SFGS_POST_LAUNCH("weld_insert", stream, 0);
  hipLaunchKernelGGL(weld_rep_kernel, grid, block, 0, stream, (const uint32_t*)w.table, w.slot_rep, w.flag, Q);
  SFGS_POST_LAUNCH("weld_rep", stream, 0);
  if (const int rc = sfgs_compact_plan(w.flag, Q, w.compact, w.compact_bytes, nullptr, stream_)) return rc;
  const SfgsCompactTensor rows[2] = {{soup, vertices, 12}, {soup_colors, colors, 12}};
  if (const int rc = sfgs_compact_rows(w.flag, Q, w.compact, rows, colors ? 2 : 1, stream_)) return rc;
  const CompactScratch plan = cp_view(w.compact, Q);
  hipLaunchKernelGGL(weld_faces_kernel, grid, block, 0, stream, (const uint32_t*)w.slot_rep, (const uint32_t*)plan.dst_index, faces, Q);
  SFGS_POST_LAUNCH("weld_faces", stream, 0);
  hipLaunchKernelGGL(mesh_sizes_kernel, dim3(1), dim3(1), 0, stream, state, (const unsigned long long*)plan.total, 0ll,
                     (const unsigned long long*)nullptr, (long long)n);
  SFGS_POST_LAUNCH("mesh_sizes", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_mesh_vet(const int32_t* faces, int64_t n, int64_t m, long long* state, void* stream_) {
  if (const int rc = mesh_check_sizes("sfgs_mesh_vet", m, n)) return rc;
  SFGS_REQUIRE(state && (faces || n == 0), SFGS_E_ARG, "sfgs_mesh_vet: NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
  hipLaunchKernelGGL(mesh_sizes_kernel, dim3(1), dim3(1), 0, stream, state, (const unsigned long long*)nullptr, (long long)m,
                     (const unsigned long long*)nullptr, (long long)n);
  SFGS_POST_LAUNCH("mesh_sizes", stream, 0);
  if (n > 0) {
    hipLaunchKernelGGL(mesh_vet_kernel, dim3(mesh_blocks(n)), dim3(MESH_THREADS), 0, stream, faces, (long long)n, (long long)m, state);
    SFGS_POST_LAUNCH("mesh_vet", stream, 0);
  }
  return SFGS_OK;
}

extern "C" size_t sfgs_mesh_components_scratch_bytes(int64_t m) {
  if (m < 0 || m > MESH_MAX_VERTICES) {
    sfgs::set_error("sfgs_mesh_components_scratch_bytes: %lld vertices, 0 ... 2^31 - 1", (long long)m);
    return 0;
  }
  return align_up((size_t)m * 4 + 4, 256);
}

extern "C" int sfgs_mesh_components(const int32_t* faces, int64_t n, int64_t m, int32_t* labels, int32_t* triangles,
                                    int32_t* vertices_in, long long* state, void* scratch, size_t scratch_bytes, void* stream_) {
  if (const int rc = mesh_check_sizes("sfgs_mesh_components", m, n)) return rc;
  SFGS_REQUIRE(state, SFGS_E_ARG, "sfgs_mesh_components: NULL state");
  hipStream_t stream = (hipStream_t)stream_;
  if (m == 0) {
    SFGS_REQUIRE(n == 0, SFGS_E_ARG, "sfgs_mesh_components: %lld faces over no vertex", (long long)n);
    SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
    return SFGS_OK;
  }
  SFGS_REQUIRE(labels && triangles && vertices_in && scratch && (faces || n == 0), SFGS_E_ARG, "sfgs_mesh_components: NULL argument");
  const size_t need = align_up((size_t)m * 4 + 4, 256);
  SFGS_REQUIRE(scratch_bytes >= need, SFGS_E_ARG, "mesh components scratch too small: %zu < %zu", scratch_bytes, need);
  int32_t* parent = (int32_t*)scratch;
  SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
  SFGS_CHECK_HIP(hipMemsetAsync(triangles, 0, (size_t)m * 4, stream));
  SFGS_CHECK_HIP(hipMemsetAsync(vertices_in, 0, (size_t)m * 4, stream));
  const dim3 block(MESH_THREADS), vgrid(mesh_blocks(m)), fgrid(mesh_blocks(n));
  hipLaunchKernelGGL(cc_init_kernel, vgrid, block, 0, stream, parent, (long long)m);
  SFGS_POST_LAUNCH("cc_init", stream, 0);
  if (n > 0) {
    hipLaunchKernelGGL(cc_hook_kernel, fgrid, block, 0, stream, faces, (long long)n, (long long)m, parent, state);
    SFGS_POST_LAUNCH("cc_hook", stream, 0);
  }
  hipLaunchKernelGGL(cc_label_kernel, vgrid, block, 0, stream, (const int32_t*)parent, (long long)m, labels, vertices_in, state);
  SFGS_POST_LAUNCH("cc_label", stream, 0);
  if (n > 0) {
    hipLaunchKernelGGL(cc_faces_kernel, fgrid, block, 0, stream, faces, (long long)n, (long long)m, (const int32_t*)labels, triangles);
    SFGS_POST_LAUNCH("cc_faces", stream, 0);
  }
  return SFGS_OK;
}

extern "C" size_t sfgs_mesh_clean_scratch_bytes(int64_t m, int64_t n) {
  if (m < 0 || m > MESH_MAX_VERTICES || n < 0 || n > MESH_MAX_TRIANGLES) {
    sfgs::set_error("sfgs_mesh_clean_scratch_bytes: %lld vertices, %lld triangles", (long long)m, (long long)n);
    return 0;
  }
  return clean_view(nullptr, m, n).total;
}

extern "C" int sfgs_mesh_clean(const float* vertices, const float* colors, const int32_t* faces, int64_t m, int64_t n,
                               const int32_t* labels, const unsigned char* keep_root, int32_t drop_degenerate, float* vertices_out,
                               float* colors_out, int32_t* faces_out, long long* state, void* scratch, size_t scratch_bytes,
                               void* stream_) {
  if (const int rc = mesh_check_sizes("sfgs_mesh_clean", m, n)) return rc;
  SFGS_REQUIRE(state && scratch, SFGS_E_ARG, "sfgs_mesh_clean: NULL state or scratch");
  SFGS_REQUIRE((colors == nullptr) == (colors_out == nullptr), SFGS_E_ARG, "sfgs_mesh_clean: colors and colors_out come together");
  SFGS_REQUIRE(drop_degenerate == 0 || drop_degenerate == 1, SFGS_E_ARG, "sfgs_mesh_clean: drop_degenerate %d", drop_degenerate);
  SFGS_REQUIRE(m > 0 || n == 0, SFGS_E_ARG, "sfgs_mesh_clean: %lld faces over no vertex", (long long)n);
  SFGS_REQUIRE(m == 0 || (vertices && vertices_out && labels && keep_root), SFGS_E_ARG, "sfgs_mesh_clean: NULL vertex argument");
  SFGS_REQUIRE(n == 0 || (faces && faces_out), SFGS_E_ARG, "sfgs_mesh_clean: NULL face argument");
  const CleanScratch c = clean_view(scratch, m, n);
  SFGS_REQUIRE(scratch_bytes >= c.total, SFGS_E_ARG, "mesh clean scratch too small: %zu < %zu", scratch_bytes, c.total);
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
  SFGS_CHECK_HIP(hipMemsetAsync(c.keep_vertex, 0, (size_t)m + 1, stream));
  const dim3 block(MESH_THREADS), fgrid(mesh_blocks(n));
  if (n > 0) {
    hipLaunchKernelGGL(clean_mark_kernel, fgrid, block, 0, stream, faces, (long long)n, (long long)m, labels, keep_root,
                       (int)drop_degenerate, c.keep_face, c.keep_vertex, state);
    SFGS_POST_LAUNCH("clean_mark", stream, 0);
  }
  if (const int rc = sfgs_compact_plan(c.keep_vertex, m, c.plan_vertex, c.plan_vertex_bytes, nullptr, stream_)) return rc;
  if (const int rc = sfgs_compact_plan(c.keep_face, n, c.plan_face, c.plan_face_bytes, nullptr, stream_)) return rc;
  const SfgsCompactTensor rows[2] = {{vertices, vertices_out, 12}, {colors, colors_out, 12}};
  if (const int rc = sfgs_compact_rows(c.keep_vertex, m, c.plan_vertex, rows, colors ? 2 : 1, stream_)) return rc;
  const CompactScratch pv = cp_view(c.plan_vertex, m), pf = cp_view(c.plan_face, n);
  if (n > 0) {
    hipLaunchKernelGGL(clean_faces_kernel, fgrid, block, 0, stream, faces, (long long)n, (const unsigned char*)c.keep_face,
                       (const uint32_t*)pf.dst_index, (const uint32_t*)pv.dst_index, faces_out);
    SFGS_POST_LAUNCH("clean_faces", stream, 0);
  }
  hipLaunchKernelGGL(mesh_sizes_kernel, dim3(1), dim3(1), 0, stream, state, (const unsigned long long*)pv.total, 0ll,
                     (const unsigned long long*)pf.total, 0ll);
  SFGS_POST_LAUNCH("mesh_sizes", stream, 0);
  return SFGS_OK;
}
