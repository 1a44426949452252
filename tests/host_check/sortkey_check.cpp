// Host view of the short-list sort's 32-bit key (raster_math.h: sortkey_*), built by g++ two ways (tests/test_sortkey_host.py):
// as a shared library whose entry points numpy drives, and -- with -DSORTKEY_MAIN -- as a stand-alone program that walks the
// key's edge cases itself (the build that runs under the host sanitizers).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../skyfall-gs_amd/csrc/raster_math.h"

using namespace sfgs;

extern "C" {
uint32_t sk_pad(void) { return SORTKEY_PAD; }
uint32_t sk_max_range(int pos_bits) { return sortkey_max_range(pos_bits); }
int sk_fits(uint32_t lo, uint32_t hi, int pos_bits) { return sortkey_fits(lo, hi, pos_bits) ? 1 : 0; }
void sk_pack(const uint32_t* depth_bits, int n, uint32_t min_bits, int pos_bits, uint32_t* keys) {
  for (int i = 0; i < n; ++i) keys[i] = sortkey_pack(depth_bits[i], min_bits, (uint32_t)i, pos_bits);
}
void sk_unpack(const uint32_t* keys, int n, int pos_bits, uint32_t* pos, uint32_t* rel, int32_t* is_pad) {
  for (int i = 0; i < n; ++i) {
    pos[i] = sortkey_pos(keys[i], pos_bits);
    rel[i] = sortkey_rel(keys[i], pos_bits);
    is_pad[i] = sortkey_is_padding(keys[i]) ? 1 : 0;
  }
}
int sk_same_depth(uint32_t a, uint32_t b, int pos_bits) { return sortkey_same_depth(a, b, pos_bits) ? 1 : 0; }
}

#ifdef SORTKEY_MAIN
static int g_fail = 0, g_lists = 0;
#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++g_fail; } \
  } while (0)

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// one list: the keys' order must be the order of (depth bits, pos), the unpacked fields what went in
static void check_list(const std::vector<uint32_t>& d, int pb) {
  const int n = (int)d.size();
  const uint32_t lo = *std::min_element(d.begin(), d.end()), hi = *std::max_element(d.begin(), d.end());
  if (!sortkey_fits(lo, hi, pb)) return;
  ++g_lists;
  std::vector<uint32_t> k(n);
  sk_pack(d.data(), n, lo, pb, k.data());
  for (int i = 0; i < n; ++i) {
    EXPECT(sortkey_pos(k[i], pb) == (uint32_t)i && sortkey_rel(k[i], pb) == d[i] - lo);
    EXPECT(!sortkey_is_padding(k[i]) && k[i] < SORTKEY_PAD);
    EXPECT(sortkey_rel(k[i], pb) < sortkey_rel(SORTKEY_PAD, pb));   // strictly below the padding's rel value
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const bool by_key = k[i] < k[j];
      const bool by_depth_pos = d[i] < d[j] || (d[i] == d[j] && i < j);
      EXPECT(by_key == by_depth_pos);
      EXPECT(sortkey_same_depth(k[i], k[j], pb) == (d[i] == d[j]));
    }
}

int main() {
  for (int pb : {9, 10}) {
    const int cap = 1 << pb;
    const uint32_t R = sortkey_max_range(pb);
    EXPECT(R == (1u << (32 - pb)) - 2u);
    // the range one below, at and one above the limit
    const uint32_t base = bits_of(1.0f);
    EXPECT(sortkey_fits(base, base + R - 1u, pb) && sortkey_fits(base, base + R, pb) && !sortkey_fits(base, base + R + 1u, pb));
    EXPECT(sortkey_fits(base, base, pb));
    // the largest real key (widest range, last position) against the padding
    const uint32_t top = sortkey_pack(base + R, base, (uint32_t)cap - 1u, pb);
    EXPECT(top < SORTKEY_PAD && !sortkey_is_padding(top) && sortkey_is_padding(SORTKEY_PAD));
    EXPECT(!sortkey_same_depth(top, SORTKEY_PAD, pb));
    EXPECT(sortkey_pos(top, pb) == (uint32_t)cap - 1u && sortkey_rel(top, pb) == R);
    // adjacent bit patterns, both orders of position
    check_list({base + 1u, base, base + 2u, base + 1u, base}, pb);
    // the full range in one list, entries in the first and the last position
    {
      std::vector<uint32_t> d(cap, base + R / 2u);
      d[0] = base + R; d[cap - 1] = base; d[1] = base + R - 1u; d[cap - 2] = base + 1u;
      check_list(d, pb);
    }
    // random depths (a fixed LCG): within one binade, across a few, and all equal
    uint32_t s = 12345u + (uint32_t)pb;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    for (int rep = 0; rep < 50; ++rep) {
      const int n = 1 + (int)(rnd() % 200u);
      const float z0 = 0.2f + (float)(rnd() % 1000u) * 0.37f;
      const float span = rep % 3 == 0 ? 0.001f : rep % 3 == 1 ? 0.3f * z0 : 0.f;
      std::vector<uint32_t> d(n);
      for (int i = 0; i < n; ++i) d[i] = bits_of(z0 + span * (float)(rnd() % 4096u) / 4096.f);
      check_list(d, pb);
    }
  }
  // what the far-camera scenes rely on: a tile's depths inside one binade fit 9 position bits
  EXPECT(sortkey_fits(bits_of(250.f), bits_of(350.f), 9));
  EXPECT(!sortkey_fits(bits_of(1.f), bits_of(300.f), 9) && !sortkey_fits(bits_of(1.f), bits_of(300.f), 10));
  EXPECT(g_lists >= 80);   // most of the lists above fit and were compared
  if (g_fail) { printf("%d failures\n", g_fail); return 1; }
  printf("sortkey OK\n");
  return 0;
}
#endif
