// Host build of csrc/mesh_math.h (g++ -ffp-contract=off, no HIP) for the decimation, the adjacency and the vertex normals of
// csrc/mesh.hip, driven by plain sequential loops over the SAME per-element functions: the cell of a vertex and its fixed point,
// the table over the cell keys (inserted in ascending order, so the first of a key claims its slot), the integer means, the
// sorted triple of a face, the face normal and the normalisation. tests/mesh_simplify_hostcheck.py is the ctypes front-end.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../skyfall-gs_amd/csrc/mesh_math.h"

using namespace sfgs;

namespace {

// rep[q] = the smallest q' with the same twelve-byte key among the records that are not skipped (MESH_EMPTY for a skipped one);
// false when a probe ran through the whole table (it cannot)
bool representatives(const uint32_t* words, const unsigned char* skip, long long Q, std::vector<uint32_t>& rep) {
  const unsigned long long slots = mesh_key_slots(Q);
  const uint32_t mask = (uint32_t)(slots - 1);
  std::vector<uint32_t> table(slots, MESH_EMPTY);
  rep.assign(Q, MESH_EMPTY);
  for (long long q = 0; q < Q; ++q) {
    if (skip[q]) continue;
    const MeshKey key = mesh_key(words, q);
    uint32_t s = mesh_hash(key) & mask;
    unsigned long long trip = 0;
    for (; trip < slots; ++trip) {
      if (table[s] == MESH_EMPTY) { table[s] = (uint32_t)q; break; }
      if (mesh_key_equal(mesh_key(words, table[s]), key)) break;
      s = (s + 1u) & mask;
    }
    if (trip == slots) return false;
    rep[q] = table[s];
  }
  return true;
}

}  // namespace

extern "C" {

unsigned long long msc_key_slots(long long keys) { return mesh_key_slots(keys); }

int msc_cell_axis(float x, double origin, double cell, int32_t* i, unsigned long long* p) {
  uint64_t pp;
  const bool ok = mesh_cell_axis(x, origin, cell, i, &pp);
  *p = pp;
  return ok ? 1 : 0;
}

unsigned long long msc_color_fix(float x) { return mesh_color_fix(x); }

// vertices / colors (or NULL) [m][3], faces [n][3] -> vertices_out / colors_out [m][3], faces_out [n][3], vertex_map [m];
// sizes_out: the vertices and faces kept, the status. Returns 0, or -1 when a probe ran through its table.
int msc_decimate(const float* vertices, const float* colors, const int32_t* faces, long long m, long long n, double cell,
                 const double* origin, int drop_duplicates, float* vertices_out, float* colors_out, int32_t* faces_out,
                 int32_t* vertex_map, long long* sizes_out) {
  unsigned status = 0;
  std::vector<int32_t> cells(3 * m);
  std::vector<uint64_t> fix(3 * m);
  std::vector<unsigned char> bad(m);
  for (long long v = 0; v < m; ++v) {
    bool ok = true;
    for (int a = 0; a < 3; ++a) ok = mesh_cell_axis(vertices[3 * v + a], origin[a], cell, &cells[3 * v + a], &fix[3 * v + a]) && ok;
    if (!ok) { cells[3 * v] = cells[3 * v + 1] = cells[3 * v + 2] = 0; status |= MESH_ST_BAD_VERTEX; }
    bad[v] = ok ? 0 : 1;
  }
  std::vector<uint32_t> rep;
  if (!representatives((const uint32_t*)cells.data(), bad.data(), m, rep)) return -1;
  std::vector<int32_t> cluster_of(m, -1), first;
  for (long long v = 0; v < m; ++v)
    if (rep[v] == (uint32_t)v) { cluster_of[v] = (int32_t)first.size(); first.push_back((int32_t)v); }
  const long long K = (long long)first.size();
  std::vector<uint32_t> count(K, 0);
  std::vector<uint64_t> sums(3 * K, 0), color_sums(3 * K, 0);
  for (long long v = 0; v < m; ++v) {
    if (bad[v]) continue;
    const int32_t k = cluster_of[v] = cluster_of[rep[v]];
    ++count[k];
    for (int a = 0; a < 3; ++a) {
      sums[3 * k + a] += fix[3 * v + a];
      if (colors) color_sums[3 * k + a] += mesh_color_fix(colors[3 * v + a]);
    }
  }
  std::vector<int32_t> g(3 * n, 0);
  std::vector<uint32_t> keys(3 * n, 0);
  std::vector<unsigned char> skip(n, 1), keep_face(n, 0), keep_cluster(K, 0);
  for (long long t = 0; t < n; ++t) {
    const int32_t a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
    if (!(mesh_index_ok(a, m) && mesh_index_ok(b, m) && mesh_index_ok(c, m))) { status |= MESH_ST_BAD_INDEX; continue; }
    const int32_t ga = cluster_of[a], gb = cluster_of[b], gc = cluster_of[c];
    if (ga < 0 || gb < 0 || gc < 0 || mesh_face_degenerate(ga, gb, gc)) continue;
    g[3 * t] = ga; g[3 * t + 1] = gb; g[3 * t + 2] = gc;
    mesh_sorted_triple(ga, gb, gc, &keys[3 * t]);
    skip[t] = 0;
  }
  std::vector<uint32_t> face_rep;
  if (!representatives(keys.data(), skip.data(), n, face_rep)) return -1;
  for (long long t = 0; t < n; ++t) {
    keep_face[t] = !skip[t] && (!drop_duplicates || face_rep[t] == (uint32_t)t);
    if (keep_face[t]) for (int c = 0; c < 3; ++c) keep_cluster[g[3 * t + c]] = 1;
  }
  std::vector<int32_t> rank(K, -1);
  long long kept_v = 0, kept_f = 0;
  for (long long k = 0; k < K; ++k) {
    if (!keep_cluster[k]) continue;
    const long long r = rank[k] = (int32_t)kept_v++;
    const int32_t f = first[k];
    if (count[k] == 1) {
      memcpy(vertices_out + 3 * r, vertices + 3 * f, 12);
      if (colors) memcpy(colors_out + 3 * r, colors + 3 * f, 12);
      continue;
    }
    for (int a = 0; a < 3; ++a) {
      vertices_out[3 * r + a] = mesh_cell_resolve(cells[3 * f + a], sums[3 * k + a], count[k], origin[a], cell);
      if (colors) colors_out[3 * r + a] = mesh_color_resolve(color_sums[3 * k + a], count[k]);
    }
  }
  for (long long t = 0; t < n; ++t) {
    if (!keep_face[t]) continue;
    for (int c = 0; c < 3; ++c) faces_out[3 * kept_f + c] = rank[g[3 * t + c]];
    ++kept_f;
  }
  for (long long v = 0; v < m; ++v) vertex_map[v] = cluster_of[v] >= 0 ? rank[cluster_of[v]] : -1;
  sizes_out[0] = kept_v; sizes_out[1] = kept_f; sizes_out[2] = status;
  return 0;
}

// offsets [m + 1], records [3 n]: a counting sort in ascending record order
int msc_vertex_faces(const int32_t* faces, long long n, long long m, int32_t* offsets, int32_t* records) {
  std::vector<long long> cursor(m + 1, 0);
  for (long long r = 0; r < 3 * n; ++r) {
    if (!mesh_index_ok(faces[r], m)) return -1;
    ++cursor[faces[r] + 1];
  }
  for (long long v = 0; v < m; ++v) cursor[v + 1] += cursor[v];
  for (long long v = 0; v <= m; ++v) offsets[v] = (int32_t)cursor[v];
  for (long long r = 0; r < 3 * n; ++r) records[cursor[faces[r]]++] = (int32_t)r;
  return 0;
}

void msc_vertex_normals(const float* vertices, const int32_t* faces, long long m, long long n, const int32_t* offsets,
                        const int32_t* records, float* normals) {
  for (long long v = 0; v < m; ++v) {
    double N[3] = {0.0, 0.0, 0.0};
    for (long long j = offsets[v]; j < offsets[v + 1]; ++j) {
      const long long t = records[j] / 3;
      double fn[3];
      mesh_face_normal(vertices + 3ll * faces[3 * t], vertices + 3ll * faces[3 * t + 1], vertices + 3ll * faces[3 * t + 2], fn);
      N[0] = N[0] + fn[0]; N[1] = N[1] + fn[1]; N[2] = N[2] + fn[2];
    }
    mesh_normalize(N, normals + 3 * v);
  }
}

}  // extern "C"
