// mesh_math.h -- what the mesh kernels (mesh.hip) decide per element, written once for the device and for the host build that
// tests/host_check/mesh_check.cpp drives sequentially: the vertex key and its hash, the table's size, the face rules.
// Integers only; nothing here touches memory but the three words of a key.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MESH_HD __host__ __device__ __forceinline__
#else
#define MESH_HD inline
#endif

namespace sfgs {

constexpr uint32_t MESH_EMPTY = 0xffffffffu;          // a hash slot that holds no soup vertex index (3 n <= 3 * 2^29 < this)
constexpr long long MESH_MAX_TRIANGLES = 1ll << 29;   // 3 n fits int32
constexpr long long MESH_MAX_VERTICES = 0x7fffffffll;
constexpr int MESH_CAS_RETRIES = 1 << 16;             // hooks that may fail in a row on one edge before the kernel gives up
// status bits (state word 2 of a mesh, word 1 of a component result): 0 = everything ran to its end
enum { MESH_ST_PROBE_BOUND = 1, MESH_ST_FIND_BOUND = 2, MESH_ST_CAS_BOUND = 4, MESH_ST_BAD_INDEX = 8 };

// A vertex key is the three 32-bit words of its position, compared as bit patterns: -0.0 != +0.0, NaNs equal when their bits are.
struct MeshKey { uint32_t w[3]; };

MESH_HD MeshKey mesh_key(const uint32_t* soup_words, long long q) {
  MeshKey k;
  k.w[0] = soup_words[3 * q]; k.w[1] = soup_words[3 * q + 1]; k.w[2] = soup_words[3 * q + 2];
  return k;
}
MESH_HD bool mesh_key_equal(const MeshKey& a, const MeshKey& b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2]; }

// murmur3's 32-bit finaliser over a running mix of the three words
MESH_HD uint32_t mesh_mix(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
MESH_HD uint32_t mesh_hash(const MeshKey& k) {
  uint32_t h = mesh_mix(k.w[0] ^ 0x9e3779b9u);
  h = mesh_mix(h ^ k.w[1] * 0x7feb352du);      // (the product binds first: the word is spread before it is folded in)
  h = mesh_mix(h ^ k.w[2] * 0x846ca68bu);
  return h;
}

// slots of the weld's table for n triangles: the power of two >= 2 * 3 n, at least 64 (load factor <= 1/2)
MESH_HD unsigned long long mesh_weld_slots(long long n) {
  unsigned long long s = 64;
  while (s < 6ull * (unsigned long long)n) s <<= 1;
  return s;
}

MESH_HD bool mesh_index_ok(int32_t v, long long m) { return v >= 0 && (long long)v < m; }
MESH_HD bool mesh_face_degenerate(int32_t a, int32_t b, int32_t c) { return a == b || b == c || a == c; }

}  // namespace sfgs
