// map_merge_main.cpp -- CPU check of the key offset of a map merge (host/map_file.cpp: hkf_map_offset_keys, hkf_map_info_offset), a program of its own:
// tests/test_map_merge_abi_cpu.py builds it with AddressSanitizer + UBSan from map_file.cpp and runs it as a child process.  usage: map_merge_main <dir>
#include "map_file.hpp"
#include "brick_key.h"
#include <limits.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: map_merge_main <dir>\n"); return 2; }
  const int32_t LO = KF_BRICK_KEY_MIN, HI = KF_BRICK_KEY_MAX - 1;
  // a plain translation, into a second array and in place; the (z, y, x) order survives a constant
  const int32_t keys[4][3] = {{-3, 5, -7}, {0, 5, -7}, {-1, 6, -7}, {2, -9, 0}};
  const int32_t off[3] = {3, -2, 5};
  int32_t out[4][3];
  CHECK(hkf_map_offset_keys(4, &keys[0][0], off, &out[0][0]));
  for (int i = 0; i < 4; ++i) for (int k = 0; k < 3; ++k) CHECK(out[i][k] == keys[i][k] + off[k]);
  int32_t same[4][3];
  memcpy(same, keys, sizeof(keys));
  CHECK(hkf_map_offset_keys(4, &same[0][0], off, &same[0][0]) && memcmp(same, out, sizeof(out)) == 0);
  CHECK(hkf_map_offset_keys(4, &keys[0][0], nullptr, &out[0][0]) && memcmp(out, keys, sizeof(keys)) == 0);   // no offset: a copy
  CHECK(hkf_map_offset_keys(0, nullptr, off, nullptr));                                                        // nothing to do
  CHECK(!hkf_map_offset_keys(1, nullptr, off, &out[0][0]) && !hkf_map_offset_keys(1, &keys[0][0], off, nullptr));
  // the range is that of the TRANSLATED key, on every axis and at both ends; a refusal writes nothing, not even the keys before the bad one
  for (int axis = 0; axis < 3; ++axis) {
    int32_t edge[2][3] = {{1, 2, 3}, {4, 5, 6}};
    int32_t o[3] = {0, 0, 0};
    edge[1][axis] = HI - 5; o[axis] = 5;
    int32_t got[2][3];
    CHECK(hkf_map_offset_keys(2, &edge[0][0], o, &got[0][0]) && got[1][axis] == HI);
    o[axis] = 6;
    memset(got, 0x55, sizeof(got));
    int32_t before[2][3];
    memcpy(before, got, sizeof(got));
    CHECK(!hkf_map_offset_keys(2, &edge[0][0], o, &got[0][0]) && memcmp(got, before, sizeof(got)) == 0);
    edge[1][axis] = LO + 5; o[axis] = -5;
    CHECK(hkf_map_offset_keys(2, &edge[0][0], o, &got[0][0]) && got[1][axis] == LO);
    o[axis] = -6;
    CHECK(!hkf_map_offset_keys(2, &edge[0][0], o, &got[0][0]));
    // an offset that brings an out-of-range key INTO range is fine: only the translated key counts
    edge[1][axis] = HI + 10; o[axis] = -10;
    CHECK(hkf_map_offset_keys(2, &edge[0][0], o, &got[0][0]) && got[1][axis] == HI);
  }
  // sums that leave 32 bits: taken in 64, so refused and not wrapped into range
  {
    const int32_t big[1][3] = {{INT_MAX, 0, 0}};
    const int32_t up[3] = {INT_MAX, 0, 0}, wrap[3] = {INT_MIN, 0, 0};
    int32_t got[1][3];
    CHECK(!hkf_map_offset_keys(1, &big[0][0], up, &got[0][0]));               // 2^32 - 2: wraps to -2 in 32 bits
    const int32_t neg[1][3] = {{INT_MIN, 0, 0}};
    CHECK(!hkf_map_offset_keys(1, &neg[0][0], wrap, &got[0][0]));             // -2^32: wraps to 0
    CHECK(hkf_map_offset_keys(1, &big[0][0], wrap, &got[0][0]) && got[0][0] == -1);            // INT_MAX + INT_MIN = -1: in range
    const int32_t y[1][3] = {{0, INT_MAX, INT_MIN}};
    const int32_t oy[3] = {0, 1, -1};
    CHECK(!hkf_map_offset_keys(1, &y[0][0], oy, &got[0][0]));
  }
  // a file: hkf_map_info_offset is hkf_map_info plus every translated key in range
  {
    const std::string path = std::string(argv[1]) + "/edge.hkfmap";
    const int32_t fk[3][3] = {{0, 0, -4}, {HI - 2, 1, 0}, {-1, LO + 3, 2}};    // (z, y, x) ascending
    HkfMapHeader h;
    memset(&h, 0, sizeof(h));
    h.resolution = 64; h.size_m = 2.f; h.max_weight = 128.f; h.n_bricks = 3;
    const int ws = hkf_map_write(path.c_str(), h, 2, [&](uint32_t first, uint32_t count, int32_t* k, float* t, float* w, uint8_t*) {
      memcpy(k, &fk[first][0], (size_t)count * 12);
      if (t) for (size_t i = 0; i < (size_t)count * HKF_MAP_BRICK_VOX; ++i) { t[i] = 0.5f; w[i] = 1.f; }
      return true;
    });
    CHECK(ws == HKF_MAP_OK);
    HkfMapHeader g;
    const int32_t fits[3] = {2, -3, 7}, past_x[3] = {3, 0, 0}, past_y[3] = {0, -4, 0}, far[3] = {INT_MAX, INT_MAX, INT_MAX};
    CHECK(hkf_map_info_offset(path.c_str(), nullptr, &g) == HKF_MAP_OK && g.n_bricks == 3);
    CHECK(hkf_map_info_offset(path.c_str(), fits, &g) == HKF_MAP_OK && g.n_bricks == 3 && g.resolution == 64);
    memset(&g, 0, sizeof(g));
    CHECK(hkf_map_info_offset(path.c_str(), past_x, &g) == HKF_MAP_ERR_KEYS && g.n_bricks == 0);
    CHECK(hkf_map_info_offset(path.c_str(), past_y, &g) == HKF_MAP_ERR_KEYS);
    CHECK(hkf_map_info_offset(path.c_str(), far, &g) == HKF_MAP_ERR_KEYS);
    CHECK(hkf_map_info_offset(nullptr, fits, &g) == HKF_MAP_ERR_ARG && hkf_map_info_offset(path.c_str(), fits, nullptr) == HKF_MAP_ERR_ARG);
    // the records read back and translated chunk by chunk stay ascending in (z, y, x)
    std::vector<int32_t> all;
    const int rs = hkf_map_read(path.c_str(), 2, HkfMapAccept(), [&](uint32_t count, const int32_t* k, const float*, const float*, const uint8_t*) {
      std::vector<int32_t> moved((size_t)count * 3);
      if (!hkf_map_offset_keys(count, k, fits, moved.data())) return false;
      all.insert(all.end(), moved.begin(), moved.end());
      return true;
    });
    CHECK(rs == HKF_MAP_OK && all.size() == 9);
    for (size_t i = 0; i + 1 < all.size() / 3 && all.size() == 9; ++i) {
      const int32_t *a = &all[3 * i], *b = &all[3 * i + 3];
      CHECK(a[2] < b[2] || (a[2] == b[2] && (a[1] < b[1] || (a[1] == b[1] && a[0] < b[0]))));
    }
    for (int i = 0; i < 3 && all.size() == 9; ++i) for (int k = 0; k < 3; ++k) CHECK(all[3 * i + k] == fk[i][k] + fits[k]);
    remove(path.c_str());
  }
  if (fails) { printf("%d checks FAILED\n", fails); return 1; }
  printf("map merge ok\n");
  return 0;
}
