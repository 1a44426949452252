// Host build of csrc/mesh_math.h (g++ -ffp-contract=off, no HIP): the weld of csrc/mesh.hip driven by plain sequential loops
// over the SAME key, hash, slot count and probe sequence -- insert every soup vertex in ascending order (the first of a key
// claims its slot, so a slot's content is the key's representative without any fetch-min), flag the representatives, rank them,
// write V, colours and F -- and the face rules of the clean. tests/mesh_hostcheck.py is the ctypes front-end.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../skyfall-gs_amd/csrc/mesh_math.h"

using namespace sfgs;

extern "C" {

unsigned long long mc_slots(long long n) { return mesh_weld_slots(n); }

uint32_t mc_hash(uint32_t w0, uint32_t w1, uint32_t w2) {
  MeshKey k;
  k.w[0] = w0; k.w[1] = w1; k.w[2] = w2;
  return mesh_hash(k);
}

int mc_degenerate(int32_t a, int32_t b, int32_t c) { return mesh_face_degenerate(a, b, c) ? 1 : 0; }
int mc_index_ok(int32_t v, long long m) { return mesh_index_ok(v, m) ? 1 : 0; }

// soup, soup_colors (or NULL): float32 [n][3][3] -> vertices / colors [3 n][3], faces [n][3]; probes_out: slots looked at in all.
// Returns m, or -1 when a probe ran through the whole table (it cannot).
long long mc_weld(const float* soup, const float* soup_colors, long long n, float* vertices, float* colors, int32_t* faces,
                  unsigned long long* probes_out) {
  const long long Q = 3 * n;
  const unsigned long long slots = mesh_weld_slots(n);
  const uint32_t mask = (uint32_t)(slots - 1);
  const uint32_t* words = (const uint32_t*)soup;
  std::vector<uint32_t> table(slots, MESH_EMPTY), rep(Q), vid(Q);
  unsigned long long probes = 0;
  for (long long q = 0; q < Q; ++q) {
    const MeshKey key = mesh_key(words, q);
    uint32_t s = mesh_hash(key) & mask;
    unsigned long long trip = 0;
    for (; trip < slots; ++trip) {
      if (table[s] == MESH_EMPTY) { table[s] = (uint32_t)q; break; }
      if (mesh_key_equal(mesh_key(words, table[s]), key)) break;
      s = (s + 1u) & mask;
    }
    if (trip == slots) return -1;
    probes += trip + 1;
    rep[q] = table[s];
  }
  long long m = 0;
  for (long long q = 0; q < Q; ++q) {
    if (rep[q] != (uint32_t)q) continue;
    vid[q] = (uint32_t)m;
    memcpy(vertices + 3 * m, soup + 3 * q, 12);
    if (soup_colors) memcpy(colors + 3 * m, soup_colors + 3 * q, 12);
    ++m;
  }
  for (long long q = 0; q < Q; ++q) faces[q] = (int32_t)vid[rep[q]];
  if (probes_out) *probes_out = probes;
  return m;
}

}  // extern "C"
