// A main of its own around host/map_file.cpp and csrc/brick_keys_unique.h, for a sanitizer run on the CPU (tests/test_map_file_abi_cpu.py): no GPU and
// no Python in the process.  argv[1]: a directory to write into.  It writes 300 synthetic bricks through the codec in chunks of 7 (the source in a
// scrambled order), reads them back in chunks of 11 and compares every word, with and without colour; feeds the reader every truncation length of a
// 3-brick file; checks that the writer refuses duplicate and out-of-range keys; and feeds the duplicate-key check its edge cases.
#include "map_file.hpp"
#include "brick_key.h"
#include "brick_keys_unique.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int fail(const char* what, long long a = 0, long long b = 0) { std::printf("FAILED: %s (%lld, %lld)\n", what, a, b); return 1; }

struct Bricks {
  std::vector<int32_t> keys; std::vector<float> t, w; std::vector<uint8_t> c;
  explicit Bricks(uint32_t n) : keys(3 * (size_t)n), t(512 * (size_t)n), w(512 * (size_t)n), c(1536 * (size_t)n) {}
};

// entry i of the source: distinct keys with negative components, in an order that is not the file's
static Bricks synthetic(uint32_t n) {
  Bricks b(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t j = (i * 7919u) % n;                           // 7919 is prime and no factor of 300 or 3: a permutation
    b.keys[3 * i] = (int32_t)(j % 7) - 3; b.keys[3 * i + 1] = (int32_t)((j / 7) % 9) - 4; b.keys[3 * i + 2] = (int32_t)(j / 63) - 2;
    for (uint32_t k = 0; k < 512; ++k) {
      b.t[512 * (size_t)i + k] = ((k + i) & 1u ? -1.f : 1.f) * (float)((j * 512u + k) % 1000u) / 1000.f;
      b.w[512 * (size_t)i + k] = (float)((j + k) % 101u);
    }
    for (uint32_t k = 0; k < 1536; ++k) b.c[1536 * (size_t)i + k] = (uint8_t)(j * 31u + k * 7u);
  }
  return b;
}

static HkfMapHeader header(uint32_t n, bool color) {
  HkfMapHeader h;
  std::memset(&h, 0, sizeof(h));
  h.resolution = 64; h.has_color = color ? 1u : 0u; h.size_m = 2.f; h.max_weight = 128.f;
  h.origin_vox[0] = 32; h.origin_vox[1] = -8; h.origin_vox[2] = 1 << 20; h.frame_id = 5;
  for (int k = 0; k < 16; ++k) h.pose[k] = 0.25f * (float)k - 1.f;
  h.n_bricks = n; h.dropped = 3;
  return h;
}

static HkfMapFetch source(const Bricks& b, bool color) {
  return [&b, color](uint32_t first, uint32_t count, int32_t* keys, float* t, float* w, uint8_t* c) {
    std::memcpy(keys, &b.keys[3 * (size_t)first], 12 * (size_t)count);
    if (t) std::memcpy(t, &b.t[512 * (size_t)first], 2048 * (size_t)count);
    if (w) std::memcpy(w, &b.w[512 * (size_t)first], 2048 * (size_t)count);
    if (c && color) std::memcpy(c, &b.c[1536 * (size_t)first], 1536 * (size_t)count);
    return true;
  };
}

static long long order_of(const int32_t* k) { return (((long long)k[2] + (1 << 20)) << 42) | (((long long)k[1] + (1 << 20)) << 21) | ((long long)k[0] + (1 << 20)); }

static int round_trip(const std::string& path, bool color) {
  const uint32_t n = 300;
  const Bricks b = synthetic(n);
  const HkfMapHeader h = header(n, color);
  int st = hkf_map_write(path.c_str(), h, 7, source(b, color));
  if (st) return fail("write", st);
  HkfMapHeader g;
  st = hkf_map_info(path.c_str(), &g);
  if (st) return fail("info", st);
  if (g.version != 1 || g.brick_edge != 8 || g.resolution != 64 || g.has_color != (color ? 1u : 0u) || g.size_m != 2.f || g.max_weight != 128.f ||
      g.origin_vox[0] != 32 || g.origin_vox[1] != -8 || g.origin_vox[2] != (1 << 20) || g.frame_id != 5 || g.n_bricks != n || g.dropped != 3 ||
      std::memcmp(g.pose, h.pose, 64) != 0) return fail("header fields");
  uint32_t seen = 0, calls = 0; long long last = -1; int bad = 0;
  bool accepted = false;
  st = hkf_map_read(path.c_str(), 11, [&](const HkfMapHeader& f) { accepted = f.n_bricks == n; return true; },
                    [&](uint32_t count, const int32_t* keys, const float* t, const float* w, const uint8_t* c) {
    ++calls;
    if (!accepted || count == 0 || count > 11 || (color ? !c : c != nullptr)) { bad = 1; return false; }
    for (uint32_t i = 0; i < count; ++i, ++seen) {
      const long long o = order_of(keys + 3 * i);
      if (o <= last) { bad = 2; return false; }                    // ascending by (z, y, x)
      last = o;
      uint32_t src = n;                                           // where the source holds this key
      for (uint32_t s = 0; s < n; ++s) if (std::memcmp(&b.keys[3 * s], keys + 3 * i, 12) == 0) { src = s; break; }
      if (src == n) { bad = 3; return false; }
      if (std::memcmp(t + 512 * (size_t)i, &b.t[512 * (size_t)src], 2048) != 0 || std::memcmp(w + 512 * (size_t)i, &b.w[512 * (size_t)src], 2048) != 0) { bad = 4; return false; }
      if (color && std::memcmp(c + 1536 * (size_t)i, &b.c[1536 * (size_t)src], 1536) != 0) { bad = 5; return false; }
    }
    return true;
  });
  if (st || bad || seen != n || calls != (n + 10) / 11) return fail("read back", st, bad);
  // a header the caller turns down: nothing is applied
  bool applied = false;
  st = hkf_map_read(path.c_str(), 11, [](const HkfMapHeader&) { return false; }, [&](uint32_t, const int32_t*, const float*, const float*, const uint8_t*) { applied = true; return true; });
  if (st != HKF_MAP_ERR_REFUSED || applied) return fail("refused header", st, applied);
  return 0;
}

static int truncations(const std::string& dir) {
  const uint32_t n = 3;
  const Bricks b = synthetic(n);
  const std::string whole = dir + "/three.hkfmap", cut = dir + "/cut.hkfmap";
  int st = hkf_map_write(whole.c_str(), header(n, true), 2, source(b, true));
  if (st) return fail("write three", st);
  std::vector<uint8_t> bytes;
  { FILE* f = std::fopen(whole.c_str(), "rb"); if (!f) return fail("reopen"); uint8_t buf[4096]; size_t got; while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got); std::fclose(f); }
  if (bytes.size() != 128 + 3 * hkf_map_record_bytes(true)) return fail("length of three", (long long)bytes.size());
  for (size_t len = 0; len < bytes.size(); ++len) {
    { FILE* f = std::fopen(cut.c_str(), "wb"); if (!f) return fail("cut"); if (len && std::fwrite(bytes.data(), 1, len, f) != len) { std::fclose(f); return fail("cut write"); } std::fclose(f); }
    HkfMapHeader g;
    bool touched = false;
    const int si = hkf_map_info(cut.c_str(), &g);
    const int sr = hkf_map_read(cut.c_str(), 2, [&](const HkfMapHeader&) { touched = true; return true; },
                                [&](uint32_t, const int32_t*, const float*, const float*, const uint8_t*) { touched = true; return true; });
    const int want = len < 128 ? HKF_MAP_ERR_MAGIC : HKF_MAP_ERR_LENGTH;
    if (si != want || sr != want || touched) return fail("truncation", (long long)len, si);
  }
  // one byte too many, a wrong magic, another version, another brick edge
  struct { size_t at; uint8_t value; bool extra; int want; } cases[] = {{0, 0, true, HKF_MAP_ERR_LENGTH}, {0, 'X', false, HKF_MAP_ERR_MAGIC}, {8, 2, false, HKF_MAP_ERR_VERSION}, {16, 4, false, HKF_MAP_ERR_BRICK}};
  for (const auto& cs : cases) {
    std::vector<uint8_t> v = bytes;
    if (cs.extra) v.push_back(0); else v[cs.at] = cs.value;
    { FILE* f = std::fopen(cut.c_str(), "wb"); if (!f) return fail("case"); std::fwrite(v.data(), 1, v.size(), f); std::fclose(f); }
    HkfMapHeader g;
    const int si = hkf_map_info(cut.c_str(), &g);
    if (si != cs.want) return fail("foreign file", (long long)cs.at, si);
  }
  // records swapped: the keys no longer ascend; a record doubled: a key twice
  const size_t rec = (size_t)hkf_map_record_bytes(true);
  for (int twice = 0; twice < 2; ++twice) {
    std::vector<uint8_t> v = bytes;
    if (twice) std::memcpy(&v[128 + rec], &v[128], rec);
    else { std::vector<uint8_t> tmp(v.begin() + 128, v.begin() + 128 + rec); std::memcpy(&v[128], &v[128 + rec], rec); std::memcpy(&v[128 + rec], tmp.data(), rec); }
    { FILE* f = std::fopen(cut.c_str(), "wb"); if (!f) return fail("keys case"); std::fwrite(v.data(), 1, v.size(), f); std::fclose(f); }
    HkfMapHeader g;
    const int si = hkf_map_info(cut.c_str(), &g);
    if (si != HKF_MAP_ERR_KEYS) return fail("unsorted or doubled keys", twice, si);
  }
  std::remove(cut.c_str());
  return 0;
}

static int writer_refusals(const std::string& dir) {
  const std::string path = dir + "/refused.hkfmap";
  Bricks b = synthetic(4);
  std::memcpy(&b.keys[9], &b.keys[0], 12);                        // the last key = the first
  if (hkf_map_write(path.c_str(), header(4, false), 3, source(b, false)) != HKF_MAP_ERR_KEYS) return fail("duplicate key written");
  b = synthetic(4);
  b.keys[4] = 1 << 20;
  if (hkf_map_write(path.c_str(), header(4, false), 3, source(b, false)) != HKF_MAP_ERR_KEYS) return fail("out-of-range key written");
  if (FILE* f = std::fopen(path.c_str(), "rb")) { std::fclose(f); return fail("a refused file was left behind"); }
  // an empty map is a header
  if (hkf_map_write(path.c_str(), header(0, false), 3, source(b, false)) != HKF_MAP_OK) return fail("empty map");
  HkfMapHeader g;
  if (hkf_map_info(path.c_str(), &g) != HKF_MAP_OK || g.n_bricks != 0) return fail("empty map read");
  std::remove(path.c_str());
  return 0;
}

static int unique_check() {
  if (!kf_brick_keys_unique(nullptr, 0)) return fail("empty list");
  unsigned long long one[1] = {kf_brick_key_pack(-1, 0, 5)};
  if (!kf_brick_keys_unique(one, 1)) return fail("one key");
  unsigned long long two[2] = {kf_brick_key_pack(3, 3, 3), kf_brick_key_pack(3, 3, 3)};
  if (kf_brick_keys_unique(two, 2)) return fail("two equal keys");
  unsigned long long apart[5] = {kf_brick_key_pack(1, 2, 3), kf_brick_key_pack(-4, 0, 0), kf_brick_key_pack(0, 0, 0), kf_brick_key_pack(7, 7, 7), kf_brick_key_pack(1, 2, 3)};
  if (kf_brick_keys_unique(apart, 5)) return fail("equal keys far apart: neighbours after the sort");
  unsigned long long ok[4] = {kf_brick_key_pack(1, 2, 3), kf_brick_key_pack(3, 2, 1), kf_brick_key_pack(-1, -2, -3), kf_brick_key_pack((1 << 20) - 1, -(1 << 20), 0)};
  if (!kf_brick_keys_unique(ok, 4)) return fail("four distinct keys");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage: map_file_main DIR");
  const std::string dir = argv[1];
  if (round_trip(dir + "/plain.hkfmap", false) || round_trip(dir + "/colour.hkfmap", true)) return 1;
  if (truncations(dir) || writer_refusals(dir) || unique_check()) return 1;
  std::printf("map file ok\n");
  return 0;
}
