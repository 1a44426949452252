// mesh.hip -- the triangle soup of tsdf.hip finished on the device: welded into an indexed mesh, its connected components
// labelled and counted, small components / degenerate faces removed. Everything is integers and copied bytes; include/sfgs.h states
// the results in words, tests/mesh_np.py in numpy, and this file is held to that restatement byte for byte. mesh_math.h has what
// is decided per element (key, hash, face rules, cells, fixed-point means, normals), built for the host too by
// tests/host_check/mesh_check.cpp and mesh_simplify_check.cpp.
//   WELD (sfgs_mesh_weld), q = 3 t + c the flat soup vertex index, Q = 3 n:
//     1. weld_insert_kernel  a thread per q: open addressing over 32-bit slots that hold soup vertex indices (MESH_EMPTY = none),
//        linear probing from mesh_hash(key). Empty slot: compare-and-swap q in. Occupied by p: compare the soup's words at p and q
//        (the soup is read-only, so whatever index a slot ever held witnesses the slot's key); equal -> fetch_min(slot, q), done;
//        else the next slot. The thread remembers its slot. After the kernel a key's slot holds rep = the key's smallest q.
//     2. weld_rep_kernel     rep_of[q] = table[slot_of[q]] (in place), flag[q] = (rep_of[q] == q). (1 and 2: mesh_key_pass.)
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
//   DECIMATE (sfgs_mesh_decimate): vertex clustering as a second weld, held to tests/mesh_simplify_np.py byte for byte.
//     1. dec_cell_kernel     a thread per vertex: the int32 cell floor((x - origin) / cell) per axis, in float64; a vertex whose
//        cell is not finite or leaves int32 is marked bad (MESH_ST_BAD_VERTEX) and takes no further part.
//     2. weld_insert_kernel over the cells as m twelve-byte keys (bad ones skipped), weld_rep_kernel, the compaction's plan:
//        cluster ranks in order of first appearance, exactly as the weld numbers its vertices.
//     3. dec_sum_kernel      count and 64-bit fixed-point sums (position inside the cell, colour; floor(f 2^32)) per cluster by
//        integer atomics, summed first over runs of a wave's lanes that share a cluster. Integers: no order can change a bit.
//     4. dec_face_kernel     G = cluster_of[F]; bad or collapsed faces are skipped, the others leave their sorted triple; with
//        drop_duplicates weld_insert_kernel / weld_rep_kernel run again over the triples and a face stays when it is its key's
//        smallest t. dec_mark_kernel marks the clusters of kept faces.
//     5. the compaction ranks kept clusters and kept faces; dec_resolve_kernel writes a kept cluster's row from its sums (or
//        copies its one member's bytes), clean_faces_kernel moves the faces through the ranks, dec_map_kernel writes the map.
//   VERTEX_FACES (sfgs_mesh_vertex_faces): vf_count_kernel (integer atomics per corner record), an exclusive scan in the three
//     launches of the compaction's plan (the middle one is scan.h's loop), vf_fill_kernel through atomic cursors, vf_sort_kernel: a thread per vertex sorts its own
//     segment in place -- insertion sort up to MESH_SORT_SHORT records, heapsort beyond, trip bound 2 k (log2 k + 2).
//   VERTEX_NORMALS (sfgs_mesh_vertex_normals): vn_kernel, a thread per vertex walks its sorted segment and sums the faces'
//     area-weighted normals in float64 in that order: no atomics, the same bits run after run.
// Shared mutable tables (the slots, parent) are read and written, inside the kernels that mutate them, with agent-scope relaxed
// atomics only. Every probe, find and retry loop has a trip bound that valid input cannot reach (the slot count, m, MESH_CAS_RETRIES);
// reaching it sets a status bit and leaves the loop. Every index read from a face is checked against m before it is used (a bad
// one sets MESH_ST_BAD_INDEX and the face is skipped); a slot's content is a soup index < Q by construction, checked all the same.
// Integer atomics only; no float atomics, no LDS beyond the per-workgroup sums, no kernel waits for another workgroup.
// No profiler ids of its own (the compaction keeps its two).
#include "sfgs_internal.h"
#include "mesh_math.h"
#include "scan.h"

namespace sfgs {

constexpr int MESH_THREADS = 256;
// the decimation's cluster sums: per wave over runs of lanes with one cluster first; false = one set of atomics per vertex
// (tools/variants/mesh_sum_per_thread.patch builds that form for the A/B in profiles/r25_mesh_simplify_ab.txt)
constexpr bool MESH_SUM_WAVE_FIRST = true;
constexpr int MESH_WAVES = MESH_THREADS / 64;

#define MESH_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ void mesh_raise(long long* __restrict__ state, unsigned bits) {
  if (bits) __hip_atomic_fetch_or((unsigned long long*)&state[2], (unsigned long long)bits, MESH_RLX);
}

// ---- weld ------------------------------------------------------------------------------------------------------------------------
template <bool STATS>
__global__ void __launch_bounds__(MESH_THREADS)
weld_insert_kernel(const uint32_t* __restrict__ soup, long long Q, uint32_t* table, unsigned long long slots,
                   uint32_t* __restrict__ slot_of, long long* __restrict__ state, const unsigned char* __restrict__ skip) {
  const long long q = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  unsigned long long probes = 0;
  if (q < Q && skip && skip[q]) {                        // (decimation) a key that takes no part: never inserted, never a witness
    slot_of[q] = 0;
  } else if (q < Q) {
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

// skip (nullable; the decimation's mask): a skipped key has no representative (MESH_EMPTY) and no flag
__global__ void __launch_bounds__(MESH_THREADS)
weld_rep_kernel(const uint32_t* __restrict__ table, uint32_t* __restrict__ slot_rep, const unsigned char* __restrict__ skip,
                unsigned char* __restrict__ flag, long long Q) {
  const long long q = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (q >= Q) return;
  if (skip && skip[q]) { slot_rep[q] = MESH_EMPTY; flag[q] = 0; return; }
  uint32_t rep = table[slot_rep[q]];                     // the slot is < slots: weld_insert_kernel
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

// ---- decimate (vertex clustering) ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS)
dec_cell_kernel(const float* __restrict__ vertices, long long m, double ox, double oy, double oz, double cell,
                int32_t* __restrict__ cells, unsigned char* __restrict__ bad, long long* __restrict__ state) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= m) return;
  int32_t i[3];
  uint64_t p;
  bool ok = mesh_cell_axis(vertices[3 * v], ox, cell, &i[0], &p);
  ok = mesh_cell_axis(vertices[3 * v + 1], oy, cell, &i[1], &p) && ok;
  ok = mesh_cell_axis(vertices[3 * v + 2], oz, cell, &i[2], &p) && ok;
#pragma unroll
  for (int a = 0; a < 3; ++a) cells[3 * v + a] = ok ? i[a] : 0;
  bad[v] = ok ? 0 : 1;
  if (!ok) mesh_raise(state, MESH_ST_BAD_VERTEX);
}

// cluster_of[v] = the first-appearance rank of v's cluster (-1: a bad vertex); the cluster's count and fixed-point sums take v's
// share through integer atomics (order does not matter: integers), and the cluster's representative leaves its own index.
// WAVE_FIRST: neighbouring vertices of a welded soup often share a cell, so a wave first sums every RUN of consecutive lanes with
// one cluster (a segmented sum over run numbers, six exchange steps) and only the first lane of a run adds -- the same integers,
// fewer atomics on one word. Every lane takes part in the exchanges; lanes beyond m or with a bad vertex are runs of their own.
template <bool WAVE_FIRST>
__global__ void __launch_bounds__(MESH_THREADS)
dec_sum_kernel(const float* __restrict__ vertices, const float* __restrict__ colors, long long m, double ox, double oy, double oz,
               double cell, const uint32_t* __restrict__ rep_of, const uint32_t* __restrict__ rank, int32_t* __restrict__ cluster_of,
               uint32_t* count, unsigned long long* sums, unsigned long long* color_sums, int32_t* __restrict__ first) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  int32_t cid = -1;
  if (v < m) {
    const uint32_t rep = rep_of[v];
    if ((long long)rep < m) {                            // else MESH_EMPTY: bad, in no cluster
      const uint32_t r = rank[rep];
      if ((long long)r < m) {                            // a rank is < m by construction
        cid = (int32_t)r;
        if (rep == (uint32_t)v) first[cid] = (int32_t)v;
      }
    }
    cluster_of[v] = cid;
  }
  const double org[3] = {ox, oy, oz};
  unsigned long long p[3] = {0, 0, 0}, pc[3] = {0, 0, 0};
  uint32_t c = 0;
  if (cid >= 0) {
    c = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int32_t i;
      uint64_t fix;
      mesh_cell_axis(vertices[3 * v + a], org[a], cell, &i, &fix);
      p[a] = fix;
      if (colors) pc[a] = mesh_color_fix(colors[3 * v + a]);
    }
  }
  bool adds = cid >= 0;
  if (WAVE_FIRST) {
    const unsigned lane = lane_id();
    const int32_t before = __shfl_up(cid, 1);
    const bool head = lane == 0 || cid < 0 || before != cid;
    const unsigned long long heads = __ballot(head);
    const int run = __popcll(heads & (~0ull >> (63 - lane)));                        // the number of this lane's run, from 1
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int other_run = __shfl_down(run, d);
      const uint32_t oc = __shfl_down(c, d);
      unsigned long long op[3], opc[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) { op[a] = __shfl_down(p[a], d); opc[a] = colors ? __shfl_down(pc[a], d) : 0ull; }
      if (lane + d < 64 && other_run == run) {
        c += oc;
#pragma unroll
        for (int a = 0; a < 3; ++a) { p[a] += op[a]; pc[a] += opc[a]; }
      }
    }
    adds = adds && head;
  }
  if (adds) {
    __hip_atomic_fetch_add(&count[cid], c, MESH_RLX);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      __hip_atomic_fetch_add(&sums[3ull * cid + a], p[a], MESH_RLX);
      if (colors) __hip_atomic_fetch_add(&color_sums[3ull * cid + a], pc[a], MESH_RLX);
    }
  }
}

// G[t] = cluster_of[F[t]]; a face with an index out of range, a bad vertex or two equal new indices is skipped; the others leave
// their sorted triple as the key under which duplicates meet
__global__ void __launch_bounds__(MESH_THREADS)
dec_face_kernel(const int32_t* __restrict__ faces, long long n, long long m, const int32_t* __restrict__ cluster_of,
                int32_t* __restrict__ gfaces, uint32_t* __restrict__ keys, unsigned char* __restrict__ skip,
                unsigned char* __restrict__ keep, long long* __restrict__ state) {
  const long long t = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (t >= n) return;
  const int a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
  int ga = 0, gb = 0, gc = 0;
  bool ok = false;
  if (mesh_index_ok(a, m) && mesh_index_ok(b, m) && mesh_index_ok(c, m)) {
    ga = cluster_of[a]; gb = cluster_of[b]; gc = cluster_of[c];
    ok = mesh_index_ok(ga, m) && mesh_index_ok(gb, m) && mesh_index_ok(gc, m) && !mesh_face_degenerate(ga, gb, gc);
  } else {
    mesh_raise(state, MESH_ST_BAD_INDEX);
  }
  if (!ok) { ga = 0; gb = 0; gc = 0; }
  gfaces[3 * t] = ga; gfaces[3 * t + 1] = gb; gfaces[3 * t + 2] = gc;
  mesh_sorted_triple(ga, gb, gc, &keys[3 * t]);
  skip[t] = ok ? 0 : 1;
  keep[t] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(MESH_THREADS)
dec_mark_kernel(const int32_t* __restrict__ gfaces, const unsigned char* __restrict__ keep_face, long long n, long long m,
                unsigned char* __restrict__ keep_cluster) {
  const long long t = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (t >= n || !keep_face[t]) return;                   // a kept face has its three cluster ranks in range: dec_face_kernel
#pragma unroll
  for (int c = 0; c < 3; ++c) keep_cluster[gfaces[3 * t + c]] = 1;                   // every writer stores the same byte
}

// a thread per cluster rank: the row of a kept cluster, from its sums -- or, with one member, that member's bytes
__global__ void __launch_bounds__(MESH_THREADS)
dec_resolve_kernel(const uint32_t* __restrict__ vertex_words, const uint32_t* __restrict__ color_words,
                   const int32_t* __restrict__ cells, const int32_t* __restrict__ first, const uint32_t* __restrict__ count,
                   const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ color_sums,
                   const unsigned char* __restrict__ keep_cluster, const uint32_t* __restrict__ rank, long long m, double ox,
                   double oy, double oz, double cell, float* __restrict__ vertices_out, float* __restrict__ colors_out) {
  const long long k = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (k >= m || !keep_cluster[k]) return;
  const long long r = rank[k];                           // <= k
  const int32_t f = first[k];
  const uint32_t c = count[k];
  if (!mesh_index_ok(f, m) || c == 0 || r >= m) return;  // a kept cluster has a representative and members
  const double org[3] = {ox, oy, oz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (c == 1) {
      ((uint32_t*)vertices_out)[3 * r + a] = vertex_words[3ll * f + a];
      if (colors_out) ((uint32_t*)colors_out)[3 * r + a] = color_words[3ll * f + a];
    } else {
      vertices_out[3 * r + a] = mesh_cell_resolve(cells[3ll * f + a], sums[3 * k + a], c, org[a], cell);
      if (colors_out) colors_out[3 * r + a] = mesh_color_resolve(color_sums[3 * k + a], c);
    }
  }
}

__global__ void __launch_bounds__(MESH_THREADS)
dec_map_kernel(const int32_t* __restrict__ cluster_of, const unsigned char* __restrict__ keep_cluster,
               const uint32_t* __restrict__ rank, long long m, int32_t* __restrict__ vertex_map) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= m) return;
  const int32_t k = cluster_of[v];
  vertex_map[v] = mesh_index_ok(k, m) && keep_cluster[k] ? (int32_t)rank[k] : -1;
}

// ---- vertex -> face adjacency ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MESH_THREADS)
vf_count_kernel(const int32_t* __restrict__ faces, long long Q, long long m, uint32_t* count, long long* __restrict__ state) {
  const long long r = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (r >= Q) return;
  const int v = faces[r];
  if (mesh_index_ok(v, m)) __hip_atomic_fetch_add(&count[v], 1u, MESH_RLX);
  else mesh_raise(state, MESH_ST_BAD_INDEX);
}

// the exclusive scan of the counts in the three launches of the row compaction's plan: sums per CP_CHUNK, ONE workgroup over the
// sums 1024 at a time with a carry (scan.h), then the offsets (and the fill's cursors, which start at them)
__global__ void __launch_bounds__(CP_NT)
vf_chunk_sum_kernel(const uint32_t* __restrict__ count, long long m, unsigned* __restrict__ block_sum) {
  __shared__ unsigned smem[CP_NT / 64 + 1];
  const long long base = (long long)blockIdx.x * CP_CHUNK + (long long)threadIdx.x * CP_ROWS_PER_THREAD;
  unsigned c = 0;
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k) c += base + k < m ? count[base + k] : 0u;
  unsigned total;
  block_excl_scan_u32<CP_NT>(c, &total, smem);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_TOP_THREADS)
vf_scan_chunks_kernel(unsigned* __restrict__ block_sum, long long NB, int32_t* __restrict__ total_out) {
  __shared__ unsigned smem[SCAN_TOP_THREADS / 64 + 1];
  const unsigned long long total = scan_sums_excl(block_sum, NB, 1, 0ull, smem);     // <= 3 n < 2^31
  if (threadIdx.x == 0) *total_out = (int32_t)total;     // offsets[m]
}

__global__ void __launch_bounds__(CP_NT)
vf_offsets_kernel(uint32_t* __restrict__ count_cursor, long long m, const unsigned* __restrict__ block_sum,
                  int32_t* __restrict__ offsets) {
  __shared__ unsigned smem[CP_NT / 64 + 1];
  const long long base = (long long)blockIdx.x * CP_CHUNK + (long long)threadIdx.x * CP_ROWS_PER_THREAD;
  unsigned cv[CP_ROWS_PER_THREAD], c = 0;
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k) { cv[k] = base + k < m ? count_cursor[base + k] : 0u; c += cv[k]; }
  unsigned total;
  unsigned pos = block_sum[blockIdx.x] + block_excl_scan_u32<CP_NT>(c, &total, smem);
#pragma unroll
  for (int k = 0; k < CP_ROWS_PER_THREAD; ++k)
    if (base + k < m) { offsets[base + k] = (int32_t)pos; count_cursor[base + k] = pos; pos += cv[k]; }
}

__global__ void __launch_bounds__(MESH_THREADS)
vf_fill_kernel(const int32_t* __restrict__ faces, long long Q, long long m, uint32_t* cursor, int32_t* __restrict__ records) {
  const long long r = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (r >= Q) return;
  const int v = faces[r];
  if (!mesh_index_ok(v, m)) return;                      // flagged by vf_count_kernel
  const uint32_t pos = __hip_atomic_fetch_add(&cursor[v], 1u, MESH_RLX);
  if ((long long)pos < Q) records[pos] = (int32_t)r;     // inside v's segment: the counts were taken from the same faces
}

// a thread per vertex sorts its own segment ascending, in place: insertion sort up to MESH_SORT_SHORT records, heapsort beyond
// (at most 1.5 k (log2 k + 1) sift steps; the trip bound is 2 k (log2 k + 2))
__global__ void __launch_bounds__(MESH_THREADS)
vf_sort_kernel(const int32_t* __restrict__ offsets, long long m, long long Q, int32_t* __restrict__ records,
               long long* __restrict__ state) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= m) return;
  const long long lo = offsets[v], hi = offsets[v + 1];
  if (lo < 0 || hi < lo || hi > Q) { mesh_raise(state, MESH_ST_BAD_INDEX); return; }
  int32_t* a = records + lo;
  const long long k = hi - lo;
  if (k <= MESH_SORT_SHORT) {
    for (int i = 1; i < (int)k; ++i) {
      const int32_t x = a[i];
      int j = i - 1;
      for (; j >= 0 && a[j] > x; --j) a[j + 1] = a[j];
      a[j + 1] = x;
    }
    return;
  }
  int lg = 0;
  while ((1ll << (lg + 1)) <= k) ++lg;
  const long long bound = 2 * k * (lg + 2);
  long long trips = 0;
  for (long long phase = k / 2 - 1 + (k - 1); phase >= 0; --phase) {                 // build the heap, then take its top k - 1 times
    long long root, end;
    if (phase >= k - 1) { root = phase - (k - 1); end = k; }
    else {
      end = phase + 1;                                   // k - 1 ... 1
      const int32_t top = a[0]; a[0] = a[end]; a[end] = top;
      root = 0;
    }
    for (;;) {
      long long child = 2 * root + 1;
      if (child >= end) break;
      if (++trips > bound) { mesh_raise(state, MESH_ST_FIND_BOUND); return; }
      int32_t cv = a[child];
      if (child + 1 < end) { const int32_t c2 = a[child + 1]; if (c2 > cv) { cv = c2; ++child; } }
      const int32_t rv = a[root];
      if (rv >= cv) break;
      a[root] = cv; a[child] = rv;
      root = child;
    }
  }
}

// ---- vertex normals ----------------------------------------------------------------------------------------------------------------
// a thread per vertex walks its segment in ascending record order and sums the faces' area-weighted normals in float64: the
// order is the segment's, so the sum is the same bits run after run. No atomics, no LDS.
__global__ void __launch_bounds__(MESH_THREADS)
vn_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, long long m, long long n,
          const int32_t* __restrict__ offsets, const int32_t* __restrict__ records, float* __restrict__ normals,
          long long* __restrict__ state) {
  const long long v = (long long)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= m) return;
  long long lo = offsets[v], hi = offsets[v + 1];
  unsigned status = 0;
  if (lo < 0 || hi < lo || hi > 3 * n) { status = MESH_ST_BAD_INDEX; lo = hi = 0; }
  double N[3] = {0.0, 0.0, 0.0};
  for (long long j = lo; j < hi; ++j) {
    const long long r = records[j];
    if (r < 0 || r >= 3 * n) { status |= MESH_ST_BAD_INDEX; continue; }
    const long long t = r / 3;
    const int a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
    if (!(mesh_index_ok(a, m) && mesh_index_ok(b, m) && mesh_index_ok(c, m))) { status |= MESH_ST_BAD_INDEX; continue; }
    double fn[3];
    mesh_face_normal(vertices + 3ll * a, vertices + 3ll * b, vertices + 3ll * c, fn);
    N[0] = N[0] + fn[0]; N[1] = N[1] + fn[1]; N[2] = N[2] + fn[2];
  }
  mesh_normalize(N, normals + 3 * v);
  mesh_raise(state, status);
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

// One pass of the key table over Q twelve-byte keys (the weld's soup vertices, the decimation's cells, its sorted triples): the
// table emptied, every key that `skip` (nullable) does not exclude inserted, then slot_rep[q] = the smallest q with q's key and
// flag[q] = (that is q itself). rep_name: the rep launch's name in an error text.
int mesh_key_pass(const uint32_t* keys, long long Q, uint32_t* table, unsigned long long slots, uint32_t* slot_rep,
                  const unsigned char* skip, unsigned char* flag, long long* state, bool stats, const char* rep_name,
                  hipStream_t stream) {
  SFGS_CHECK_HIP(hipMemsetAsync(table, 0xff, (size_t)slots * 4, stream));
  const dim3 grid(mesh_blocks(Q)), block(MESH_THREADS);
  if (stats) hipLaunchKernelGGL(weld_insert_kernel<true>, grid, block, 0, stream, keys, Q, table, slots, slot_rep, state, skip);
  else hipLaunchKernelGGL(weld_insert_kernel<false>, grid, block, 0, stream, keys, Q, table, slots, slot_rep, state, skip);
  SFGS_POST_LAUNCH("weld_insert", stream, 0);
  hipLaunchKernelGGL(weld_rep_kernel, grid, block, 0, stream, (const uint32_t*)table, slot_rep, skip, flag, Q);
  SFGS_POST_LAUNCH(rep_name, stream, 0);
  return SFGS_OK;
}

int mesh_sizes(long long* state, const unsigned long long* a, long long av, const unsigned long long* b, long long bv,
               hipStream_t stream) {
  hipLaunchKernelGGL(mesh_sizes_kernel, dim3(1), dim3(1), 0, stream, state, a, av, b, bv);
  SFGS_POST_LAUNCH("mesh_sizes", stream, 0);
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
  const dim3 grid(mesh_blocks(Q)), block(MESH_THREADS);
  if (const int rc = mesh_key_pass((const uint32_t*)soup, Q, w.table, slots, w.slot_rep, nullptr, w.flag, state, flags & 1, "weld_rep",
                                   stream))
    return rc;
  if (const int rc = sfgs_compact_plan(w.flag, Q, w.compact, w.compact_bytes, nullptr, stream_)) return rc;
  const SfgsCompactTensor rows[2] = {{soup, vertices, 12}, {soup_colors, colors, 12}};
  if (const int rc = sfgs_compact_rows(w.flag, Q, w.compact, rows, colors ? 2 : 1, stream_)) return rc;
  const CompactScratch plan = cp_view(w.compact, Q);
  hipLaunchKernelGGL(weld_faces_kernel, grid, block, 0, stream, (const uint32_t*)w.slot_rep, (const uint32_t*)plan.dst_index, faces, Q);
  SFGS_POST_LAUNCH("weld_faces", stream, 0);
  return mesh_sizes(state, plan.total, 0, nullptr, n, stream);
}

extern "C" int sfgs_mesh_vet(const int32_t* faces, int64_t n, int64_t m, long long* state, void* stream_) {
  if (const int rc = mesh_check_sizes("sfgs_mesh_vet", m, n)) return rc;
  SFGS_REQUIRE(state && (faces || n == 0), SFGS_E_ARG, "sfgs_mesh_vet: NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
  if (const int rc = mesh_sizes(state, nullptr, m, nullptr, n, stream)) return rc;
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
  return mesh_sizes(state, pv.total, 0, pf.total, 0, stream);
}

// ---- decimate, vertex_faces, vertex_normals ----------------------------------------------------------------------------------------
namespace {

struct DecimateScratch {
  uint32_t* table;                    // [max(slots of m keys, slots of n keys)], used for the cells, then for the sorted triples
  int32_t* cells;                     // [m][3]
  unsigned char *bad, *flag, *keep_cluster;     // [m]
  uint32_t *rep_of, *count;           // [m]
  int32_t *cluster_of, *first;        // [m]
  unsigned long long *sums, *color_sums;        // [m][3]
  int32_t* gfaces;                    // [n][3]
  uint32_t* keys;                     // [n][3]
  uint32_t* face_rep;                 // [n]
  unsigned char *skip_face, *keep_face;         // [n]
  void *plan_cluster, *plan_vertex, *plan_face;
  size_t plan_m_bytes, plan_n_bytes, table_bytes, zero_bytes, total;
  char* zero_from;                    // count ... keep_cluster: one memset
};
DecimateScratch decimate_view(void* base, long long m, long long n, bool colours) {
  DecimateScratch d;
  char* p = (char*)base;
  size_t off = 0;
  const unsigned long long sv = mesh_key_slots(m), sf = mesh_key_slots(n);
  d.table_bytes = (size_t)(sv > sf ? sv : sf) * 4;
  d.table = (uint32_t*)(p + off); off += align_up(d.table_bytes, 256);
  d.cells = (int32_t*)(p + off); off += align_up((size_t)m * 12, 256);
  d.bad = (unsigned char*)(p + off); off += align_up((size_t)m + 1, 256);
  d.flag = (unsigned char*)(p + off); off += align_up((size_t)m + 1, 256);
  d.rep_of = (uint32_t*)(p + off); off += align_up((size_t)m * 4, 256);
  d.cluster_of = (int32_t*)(p + off); off += align_up((size_t)m * 4, 256);
  d.first = (int32_t*)(p + off); off += align_up((size_t)m * 4, 256);
  d.zero_from = p + off;
  const size_t zero_begin = off;
  d.count = (uint32_t*)(p + off); off += align_up((size_t)m * 4, 256);
  d.sums = (unsigned long long*)(p + off); off += align_up((size_t)m * 24, 256);
  d.color_sums = (unsigned long long*)(p + off); off += colours ? align_up((size_t)m * 24, 256) : 0;
  d.keep_cluster = (unsigned char*)(p + off); off += align_up((size_t)m + 1, 256);
  d.zero_bytes = off - zero_begin;
  d.gfaces = (int32_t*)(p + off); off += align_up((size_t)n * 12, 256);
  d.keys = (uint32_t*)(p + off); off += align_up((size_t)n * 12, 256);
  d.face_rep = (uint32_t*)(p + off); off += align_up((size_t)n * 4, 256);
  d.skip_face = (unsigned char*)(p + off); off += align_up((size_t)n + 1, 256);
  d.keep_face = (unsigned char*)(p + off); off += align_up((size_t)n + 1, 256);
  d.plan_m_bytes = cp_scratch_bytes(m); d.plan_n_bytes = cp_scratch_bytes(n);
  d.plan_cluster = p + off; off += d.plan_m_bytes;
  d.plan_vertex = p + off; off += d.plan_m_bytes;
  d.plan_face = p + off; off += d.plan_n_bytes;
  d.total = off;
  return d;
}

struct AdjacencyScratch {
  uint32_t* cursor;                   // [m] the counts, then the fill's cursors
  unsigned* block_sum;                // [cp_blocks(m)]
  size_t total;
};
AdjacencyScratch adjacency_view(void* base, long long m) {
  AdjacencyScratch a;
  char* p = (char*)base;
  size_t off = 0;
  a.cursor = (uint32_t*)(p + off); off += align_up((size_t)m * 4 + 4, 256);
  a.block_sum = (unsigned*)(p + off); off += align_up((size_t)cp_blocks(m) * 4 + 4, 256);
  a.total = off;
  return a;
}

}  // namespace

extern "C" size_t sfgs_mesh_decimate_scratch_bytes(int64_t m, int64_t n, int32_t with_colors) {
  if (m < 0 || m > MESH_MAX_VERTICES || n < 0 || n > MESH_MAX_TRIANGLES || (with_colors & ~1)) {
    sfgs::set_error("sfgs_mesh_decimate_scratch_bytes: %lld vertices, %lld triangles, with_colors %d", (long long)m, (long long)n,
                    with_colors);
    return 0;
  }
  return decimate_view(nullptr, m, n, with_colors != 0).total;
}

extern "C" int sfgs_mesh_decimate(const float* vertices, const float* colors, const int32_t* faces, int64_t m, int64_t n, double cell,
                                  double origin_x, double origin_y, double origin_z, int32_t flags, float* vertices_out,
                                  float* colors_out, int32_t* faces_out, int32_t* vertex_map, long long* state, void* scratch,
                                  size_t scratch_bytes, void* stream_) {
  if (const int rc = mesh_check_sizes("sfgs_mesh_decimate", m, n)) return rc;
  SFGS_REQUIRE(state && scratch, SFGS_E_ARG, "sfgs_mesh_decimate: NULL state or scratch");
  SFGS_REQUIRE(cell > 0.0 && cell - cell == 0.0, SFGS_E_ARG, "sfgs_mesh_decimate: cell %g, finite and > 0", cell);
  SFGS_REQUIRE(origin_x - origin_x == 0.0 && origin_y - origin_y == 0.0 && origin_z - origin_z == 0.0, SFGS_E_ARG,
               "sfgs_mesh_decimate: origin (%g, %g, %g) is not finite", origin_x, origin_y, origin_z);
  SFGS_REQUIRE((flags & ~3) == 0, SFGS_E_ARG, "sfgs_mesh_decimate: flags %d", flags);
  SFGS_REQUIRE(m == 0 || (colors == nullptr) == (colors_out == nullptr), SFGS_E_ARG,
               "sfgs_mesh_decimate: colors and colors_out come together");
  SFGS_REQUIRE(m > 0 || n == 0, SFGS_E_ARG, "sfgs_mesh_decimate: %lld faces over no vertex", (long long)n);
  SFGS_REQUIRE(m == 0 || (vertices && vertices_out), SFGS_E_ARG, "sfgs_mesh_decimate: NULL vertex argument");
  SFGS_REQUIRE(n == 0 || (faces && faces_out), SFGS_E_ARG, "sfgs_mesh_decimate: NULL face argument");
  const DecimateScratch d = decimate_view(scratch, m, n, colors != nullptr);
  SFGS_REQUIRE(scratch_bytes >= d.total, SFGS_E_ARG, "mesh decimate scratch too small: %zu < %zu", scratch_bytes, d.total);
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
  if (m == 0) return SFGS_OK;                            // no launch that indexes anything
  const bool drop_duplicates = flags & 1, stats = flags & 2;
  const dim3 block(MESH_THREADS), vgrid(mesh_blocks(m)), fgrid(mesh_blocks(n));
  const unsigned long long vslots = mesh_key_slots(m), fslots = mesh_key_slots(n);
  SFGS_CHECK_HIP(hipMemsetAsync(d.zero_from, 0, d.zero_bytes, stream));
  // clusters: cells, the weld's table over them, first-appearance ranks, sums
  hipLaunchKernelGGL(dec_cell_kernel, vgrid, block, 0, stream, vertices, (long long)m, origin_x, origin_y, origin_z, cell, d.cells,
                     d.bad, state);
  SFGS_POST_LAUNCH("dec_cell", stream, 0);
  if (const int rc = mesh_key_pass((const uint32_t*)d.cells, m, d.table, vslots, d.rep_of, d.bad, d.flag, state, stats, "dec_rep", stream))
    return rc;
  if (const int rc = sfgs_compact_plan(d.flag, m, d.plan_cluster, d.plan_m_bytes, nullptr, stream_)) return rc;
  const CompactScratch pc = cp_view(d.plan_cluster, m);
  hipLaunchKernelGGL(dec_sum_kernel<MESH_SUM_WAVE_FIRST>, vgrid, block, 0, stream, vertices, colors, (long long)m, origin_x, origin_y, origin_z, cell,
                     (const uint32_t*)d.rep_of, (const uint32_t*)pc.dst_index, d.cluster_of, d.count, d.sums, d.color_sums, d.first);
  SFGS_POST_LAUNCH("dec_sum", stream, 0);
  // faces: through the clusters, collapsed ones out, duplicates out by a second pass of the table over the sorted triples
  if (n > 0) {
    hipLaunchKernelGGL(dec_face_kernel, fgrid, block, 0, stream, faces, (long long)n, (long long)m, (const int32_t*)d.cluster_of,
                       d.gfaces, d.keys, d.skip_face, d.keep_face, state);
    SFGS_POST_LAUNCH("dec_face", stream, 0);
    if (drop_duplicates)
      if (const int rc = mesh_key_pass(d.keys, n, d.table, fslots, d.face_rep, d.skip_face, d.keep_face, state, false, "dec_rep", stream))
        return rc;
    hipLaunchKernelGGL(dec_mark_kernel, fgrid, block, 0, stream, (const int32_t*)d.gfaces, (const unsigned char*)d.keep_face,
                       (long long)n, (long long)m, d.keep_cluster);
    SFGS_POST_LAUNCH("dec_mark", stream, 0);
  }
  if (const int rc = sfgs_compact_plan(d.keep_cluster, m, d.plan_vertex, d.plan_m_bytes, nullptr, stream_)) return rc;
  if (const int rc = sfgs_compact_plan(d.keep_face, n, d.plan_face, d.plan_n_bytes, nullptr, stream_)) return rc;
  const CompactScratch pv = cp_view(d.plan_vertex, m), pf = cp_view(d.plan_face, n);
  hipLaunchKernelGGL(dec_resolve_kernel, vgrid, block, 0, stream, (const uint32_t*)vertices, (const uint32_t*)colors,
                     (const int32_t*)d.cells, (const int32_t*)d.first, (const uint32_t*)d.count, (const unsigned long long*)d.sums,
                     (const unsigned long long*)d.color_sums, (const unsigned char*)d.keep_cluster, (const uint32_t*)pv.dst_index,
                     (long long)m, origin_x, origin_y, origin_z, cell, vertices_out, colors_out);
  SFGS_POST_LAUNCH("dec_resolve", stream, 0);
  if (n > 0) {
    hipLaunchKernelGGL(clean_faces_kernel, fgrid, block, 0, stream, (const int32_t*)d.gfaces, (long long)n,
                       (const unsigned char*)d.keep_face, (const uint32_t*)pf.dst_index, (const uint32_t*)pv.dst_index, faces_out);
    SFGS_POST_LAUNCH("clean_faces", stream, 0);
  }
  if (vertex_map) {
    hipLaunchKernelGGL(dec_map_kernel, vgrid, block, 0, stream, (const int32_t*)d.cluster_of, (const unsigned char*)d.keep_cluster,
                       (const uint32_t*)pv.dst_index, (long long)m, vertex_map);
    SFGS_POST_LAUNCH("dec_map", stream, 0);
  }
  return mesh_sizes(state, pv.total, 0, pf.total, 0, stream);
}

extern "C" size_t sfgs_mesh_vertex_faces_scratch_bytes(int64_t m) {
  if (m < 0 || m > MESH_MAX_VERTICES) {
    sfgs::set_error("sfgs_mesh_vertex_faces_scratch_bytes: %lld vertices, 0 ... 2^31 - 1", (long long)m);
    return 0;
  }
  return adjacency_view(nullptr, m).total;
}

extern "C" int sfgs_mesh_vertex_faces(const int32_t* faces, int64_t n, int64_t m, int32_t* offsets, int32_t* records, long long* state,
                                      void* scratch, size_t scratch_bytes, void* stream_) {
  if (const int rc = mesh_check_sizes("sfgs_mesh_vertex_faces", m, n)) return rc;
  SFGS_REQUIRE(state && offsets && scratch, SFGS_E_ARG, "sfgs_mesh_vertex_faces: NULL state, offsets or scratch");
  SFGS_REQUIRE(m > 0 || n == 0, SFGS_E_ARG, "sfgs_mesh_vertex_faces: %lld faces over no vertex", (long long)n);
  SFGS_REQUIRE(n == 0 || (faces && records), SFGS_E_ARG, "sfgs_mesh_vertex_faces: NULL face argument");
  const AdjacencyScratch a = adjacency_view(scratch, m);
  SFGS_REQUIRE(scratch_bytes >= a.total, SFGS_E_ARG, "mesh vertex_faces scratch too small: %zu < %zu", scratch_bytes, a.total);
  hipStream_t stream = (hipStream_t)stream_;
  SFGS_CHECK_HIP(hipMemsetAsync(state, 0, 32, stream));
  if (const int rc = mesh_sizes(state, nullptr, m, nullptr, n, stream)) return rc;
  if (n == 0) {                                          // every segment is empty
    SFGS_CHECK_HIP(hipMemsetAsync(offsets, 0, ((size_t)m + 1) * 4, stream));
    return SFGS_OK;
  }
  const long long Q = 3 * (long long)n, NB = cp_blocks(m);
  const dim3 block(MESH_THREADS), vgrid(mesh_blocks(m)), rgrid(mesh_blocks(Q));
  SFGS_CHECK_HIP(hipMemsetAsync(a.cursor, 0, (size_t)m * 4, stream));
  hipLaunchKernelGGL(vf_count_kernel, rgrid, block, 0, stream, faces, Q, (long long)m, a.cursor, state);
  SFGS_POST_LAUNCH("vf_count", stream, 0);
  hipLaunchKernelGGL(vf_chunk_sum_kernel, dim3((unsigned)NB), dim3(CP_NT), 0, stream, (const uint32_t*)a.cursor, (long long)m, a.block_sum);
  hipLaunchKernelGGL(vf_scan_chunks_kernel, dim3(1), dim3(SCAN_TOP_THREADS), 0, stream, a.block_sum, NB, offsets + m);
  hipLaunchKernelGGL(vf_offsets_kernel, dim3((unsigned)NB), dim3(CP_NT), 0, stream, a.cursor, (long long)m, (const unsigned*)a.block_sum,
                     offsets);
  SFGS_POST_LAUNCH("vf_scan", stream, 0);
  hipLaunchKernelGGL(vf_fill_kernel, rgrid, block, 0, stream, faces, Q, (long long)m, a.cursor, records);
  SFGS_POST_LAUNCH("vf_fill", stream, 0);
  hipLaunchKernelGGL(vf_sort_kernel, vgrid, block, 0, stream, (const int32_t*)offsets, (long long)m, Q, records, state);
  SFGS_POST_LAUNCH("vf_sort", stream, 0);
  return SFGS_OK;
}

extern "C" int sfgs_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t m, int64_t n, const int32_t* offsets,
                                        const int32_t* records, float* normals, long long* state, void* stream_) {
  if (const int rc = mesh_check_sizes("sfgs_mesh_vertex_normals", m, n)) return rc;
  SFGS_REQUIRE(state, SFGS_E_ARG, "sfgs_mesh_vertex_normals: NULL state");
  SFGS_REQUIRE(m > 0 || n == 0, SFGS_E_ARG, "sfgs_mesh_vertex_normals: %lld faces over no vertex", (long long)n);
  SFGS_REQUIRE(m == 0 || (vertices && offsets && normals), SFGS_E_ARG, "sfgs_mesh_vertex_normals: NULL vertex argument");
  SFGS_REQUIRE(n == 0 || (faces && records), SFGS_E_ARG, "sfgs_mesh_vertex_normals: NULL face argument");
  if (m == 0) return SFGS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(vn_kernel, dim3(mesh_blocks(m)), dim3(MESH_THREADS), 0, stream, vertices, faces, (long long)m, (long long)n,
                     offsets, records, normals, state);
  SFGS_POST_LAUNCH("vn", stream, 0);
  return SFGS_OK;
}
