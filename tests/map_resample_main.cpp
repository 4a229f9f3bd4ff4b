// map_resample_main.cpp -- CPU check of the host side of a map merge under a rigid transform (csrc/rigid_keys.h: kf_rigid_valid, kf_rigid_keys,
// kf_rigid_brick_base, kf_rigid_source_table, kf_source_keys_table), a program of its own: tests/test_map_resample_abi_cpu.py builds it with
// AddressSanitizer + UBSan and runs it as a child process.  usage: map_resample_main
#include "rigid_keys.h"
#include <limits.h>
#include <stdio.h>
#include <string.h>
#include <set>
#include <vector>

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

// Rodrigues: the rotation by `deg` about the axis (x, y, z), with translation t
static void rotation(double deg, double x, double y, double z, const double t[3], double xf[12]) {
  const double n = sqrt(x * x + y * y + z * z), a = deg * M_PI / 180.0, c = cos(a), s = sin(a), k[3] = {x / n, y / n, z / n};
  const double K[3][3] = {{0, -k[2], k[1]}, {k[2], 0, -k[0]}, {-k[1], k[0], 0}};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) xf[4 * i + j] = (i == j ? c : 0.0) + s * K[i][j] + (1.0 - c) * k[i] * k[j];
    xf[4 * i + 3] = t[i];
  }
}

static bool sorted_unique_zyx(const std::vector<int32_t>& k) {
  for (size_t i = 0; i + 1 < k.size() / 3; ++i) {
    const int32_t *a = &k[3 * i], *b = &k[3 * i + 3];
    if (!(a[2] < b[2] || (a[2] == b[2] && (a[1] < b[1] || (a[1] == b[1] && a[0] < b[0]))))) return false;
  }
  return true;
}

int main() {
  const double zero[3] = {0, 0, 0};
  double I[12];
  rotation(0.0, 0, 0, 1, zero, I);
  // ---- what is a transform
  CHECK(kf_rigid_valid(I) && !kf_rigid_valid(nullptr));
  {
    double r[12];
    const double t[3] = {2.3, -1.7, 0.4};
    rotation(20.0, 1, 2, 3, t, r);
    CHECK(kf_rigid_valid(r));
    for (int i = 0; i < 12; ++i) { double bad[12]; memcpy(bad, r, sizeof(r)); bad[i] = NAN; CHECK(!kf_rigid_valid(bad)); bad[i] = INFINITY; CHECK(!kf_rigid_valid(bad)); }
    double scaled[12], mirror[12], f32[12];
    for (int i = 0; i < 12; ++i) { scaled[i] = (i % 4 == 3) ? r[i] : 1.001 * r[i]; mirror[i] = (i < 3) ? -r[i] : r[i]; f32[i] = (double)(float)r[i]; }
    CHECK(!kf_rigid_valid(scaled) && !kf_rigid_valid(mirror));
    CHECK(kf_rigid_valid(f32));                                  // a rotation rounded to fp32 is one
    double zeros[12] = {0};
    CHECK(!kf_rigid_valid(zeros));
  }
  // ---- the candidates
  const int32_t keys[3][3] = {{0, 0, 0}, {1, 0, 0}, {-3, 5, 7}};
  {
    CHECK(kf_rigid_keys(3, &keys[0][0], I, nullptr, 0) == 36 + 27);          // two x-neighbours: 4 x 3 x 3; one alone: 3^3
    std::vector<int32_t> out(63 * 3);
    CHECK(kf_rigid_keys(3, &keys[0][0], I, out.data(), 63) == 63 && sorted_unique_zyx(out));
    std::set<std::vector<int32_t>> have;
    for (int i = 0; i < 63; ++i) have.insert({out[3 * i], out[3 * i + 1], out[3 * i + 2]});
    for (int e = 0; e < 3; ++e) for (int z = -1; z <= 1; ++z) for (int y = -1; y <= 1; ++y) for (int x = -1; x <= 1; ++x)
      CHECK(have.count({keys[e][0] + x, keys[e][1] + y, keys[e][2] + z}) == 1);
    // cap: only the first `cap` are written, the count is the whole list's
    std::vector<int32_t> few(5 * 3 + 3, 0x55555555);
    CHECK(kf_rigid_keys(3, &keys[0][0], I, few.data(), 5) == 63 && memcmp(few.data(), out.data(), 15 * 4) == 0 && few[15] == 0x55555555);
    CHECK(kf_rigid_keys(0, nullptr, I, nullptr, 0) == 0);
    CHECK(kf_rigid_keys(3, nullptr, I, nullptr, 0) == -1 && kf_rigid_keys(3, &keys[0][0], nullptr, nullptr, 0) == -1 && kf_rigid_keys(3, &keys[0][0], I, nullptr, 4) == -1);
  }
  {
    // a translation by whole bricks moves the list; a general transform keeps every brick a transformed source voxel centre falls into
    const double t[3] = {8, -16, 24};
    double xf[12];
    rotation(0.0, 0, 0, 1, t, xf);
    std::vector<int32_t> a(63 * 3), b(63 * 3);
    CHECK(kf_rigid_keys(3, &keys[0][0], I, a.data(), 63) == 63 && kf_rigid_keys(3, &keys[0][0], xf, b.data(), 63) == 63);
    for (int i = 0; i < 63; ++i) CHECK(b[3 * i] == a[3 * i] + 1 && b[3 * i + 1] == a[3 * i + 1] - 2 && b[3 * i + 2] == a[3 * i + 2] + 3);
    const double t2[3] = {2.3, -1.7, 0.4};
    rotation(20.0, 1, 2, 3, t2, xf);
    const int64_t n = kf_rigid_keys(3, &keys[0][0], xf, nullptr, 0);
    CHECK(n > 0);
    std::vector<int32_t> c((size_t)n * 3);
    CHECK(kf_rigid_keys(3, &keys[0][0], xf, c.data(), n) == n && sorted_unique_zyx(c));
    std::set<std::vector<int32_t>> have;
    for (int64_t i = 0; i < n; ++i) have.insert({c[3 * i], c[3 * i + 1], c[3 * i + 2]});
    for (int e = 0; e < 3; ++e) for (int v = 0; v < 512; ++v) {
      const double s[3] = {8.0 * keys[e][0] + (v & 7) + 0.5, 8.0 * keys[e][1] + ((v >> 3) & 7) + 0.5, 8.0 * keys[e][2] + (v >> 6) + 0.5};
      std::vector<int32_t> k(3);
      for (int i = 0; i < 3; ++i) k[i] = (int32_t)floor((xf[4 * i] * s[0] + xf[4 * i + 1] * s[1] + xf[4 * i + 2] * s[2] + xf[4 * i + 3] - 0.5) / 8.0);
      CHECK(have.count(k) == 1);
    }
  }
  {
    // the key range: the last brick's +1 neighbour lies outside, so does anything a far translation pushes out; int32 extremes do not wrap
    const int32_t HI = KF_BRICK_KEY_MAX - 1, LO = KF_BRICK_KEY_MIN;
    const int32_t edge[1][3] = {{HI, 0, 0}}, inside[1][3] = {{HI - 1, LO + 1, 0}}, wild[1][3] = {{INT_MAX, INT_MIN, 0}};
    CHECK(kf_rigid_keys(1, &edge[0][0], I, nullptr, 0) == -1 && kf_rigid_keys(1, &inside[0][0], I, nullptr, 0) == 27 && kf_rigid_keys(1, &wild[0][0], I, nullptr, 0) == -1);
    double far[12];
    const double t[3] = {8.0 * (1 << 20), 0, 0}, huge[3] = {1e300, -1e300, 1e300};
    rotation(0.0, 0, 0, 1, t, far);
    CHECK(kf_rigid_keys(3, &keys[0][0], far, nullptr, 0) == -1);
    rotation(0.0, 0, 0, 1, huge, far);
    CHECK(kf_rigid_keys(3, &keys[0][0], far, nullptr, 0) == -1);
  }
  // ---- a candidate's base corner
  {
    int32_t ib[3];
    float fb[3];
    const int32_t K[3] = {2, -1, 0};
    CHECK(kf_rigid_brick_base(I, K, ib, fb) && ib[0] == 16 && ib[1] == -8 && ib[2] == 0 && fb[0] == 0.f && fb[1] == 0.f && fb[2] == 0.f);
    const double t[3] = {3, -5, 12.25};
    double xf[12];
    rotation(0.0, 0, 0, 1, t, xf);
    CHECK(kf_rigid_brick_base(xf, K, ib, fb) && ib[0] == 13 && ib[1] == -3 && ib[2] == -13 && fb[0] == 0.f && fb[1] == 0.f && fb[2] == 0.75f);
    const double eps[3] = {1e-12, 0, 0};                         // c = 16 - 1e-12: the fraction rounds to 1.0f and moves into the integer
    rotation(0.0, 0, 0, 1, eps, xf);
    CHECK(kf_rigid_brick_base(xf, K, ib, fb) && ib[0] == 16 && fb[0] == 0.f);
    const double away[3] = {1e12, 0, 0};
    rotation(0.0, 0, 0, 1, away, xf);
    CHECK(!kf_rigid_brick_base(xf, K, ib, fb));
  }
  // ---- the source table: every key is found from its hash on before a free entry, no other key is
  {
    std::vector<int32_t> many;
    for (int z = -3; z < 4; ++z) for (int y = -2; y < 3; ++y) for (int x = 0; x < 9; ++x) { many.push_back(x * 37 - 100); many.push_back(y); many.push_back(z * 1000); }
    const uint32_t n = (uint32_t)(many.size() / 3);
    std::vector<unsigned long long> tkey;
    std::vector<unsigned> tslot;
    const uint32_t mask = kf_rigid_source_table(n, many.data(), tkey, tslot);
    CHECK(tkey.size() == (size_t)mask + 1 && tslot.size() == tkey.size() && (tkey.size() & mask) == 0 && tkey.size() >= 2 * (size_t)n && tkey.size() < 4 * (size_t)n);
    auto find = [&](unsigned long long key) {
      for (uint32_t p = 0, h = kf_brick_key_hash(key, mask); p <= mask; ++p, h = (h + 1u) & mask) {
        if (tkey[h] == key) return (int64_t)tslot[h];
        if (tkey[h] == KF_BRICK_KEY_EMPTY) break;
      }
      return (int64_t)-1;
    };
    for (uint32_t e = 0; e < n; ++e) CHECK(find(kf_brick_key_pack(many[3 * e], many[3 * e + 1], many[3 * e + 2])) == (int64_t)e);
    CHECK(find(kf_brick_key_pack(1, 1, 1)) == -1 && find(kf_brick_key_pack(-100, 0, 1)) == -1);
    CHECK(kf_rigid_source_table(0, nullptr, tkey, tslot) == 1 && tkey.size() == 2 && tkey[0] == KF_BRICK_KEY_EMPTY && tkey[1] == KF_BRICK_KEY_EMPTY);
  }
  // ---- the source keys of an entry point: in range, each once, then the table
  {
    std::vector<unsigned long long> tkey;
    std::vector<unsigned> tslot;
    uint32_t mask = 77;
    CHECK(kf_source_keys_table(0, nullptr, tkey, tslot, mask) && mask == 1 && tkey.size() == 2 && tkey[0] == KF_BRICK_KEY_EMPTY && tkey[1] == KF_BRICK_KEY_EMPTY);
    const int32_t HI = KF_BRICK_KEY_MAX - 1, LO = KF_BRICK_KEY_MIN;
    for (int j = 0; j < 3; ++j) {                                // each component at either end of the range, and one past it
      int32_t k[2][3] = {{5, -6, 7}, {0, 0, 0}};
      k[0][j] = HI; k[1][j] = LO;
      mask = 77;
      CHECK(kf_source_keys_table(2, &k[0][0], tkey, tslot, mask) && mask == 3 && tkey.size() == 4);
      const std::vector<unsigned long long> held = tkey;
      k[0][j] = HI + 1; mask = 77;
      CHECK(!kf_source_keys_table(2, &k[0][0], tkey, tslot, mask) && mask == 77 && tkey == held);   // refused: nothing written
      k[0][j] = HI; k[1][j] = LO - 1;
      CHECK(!kf_source_keys_table(2, &k[0][0], tkey, tslot, mask) && mask == 77 && tkey == held);
      k[1][j] = INT_MIN; k[0][j] = INT_MAX;
      CHECK(!kf_source_keys_table(2, &k[0][0], tkey, tslot, mask));
    }
    const int32_t twice[3][3] = {{1, 2, 3}, {-1, -2, -3}, {1, 2, 3}}, once[3][3] = {{1, 2, 3}, {-1, -2, -3}, {1, 2, 4}};
    mask = 77;
    CHECK(!kf_source_keys_table(3, &twice[0][0], tkey, tslot, mask) && mask == 77);
    CHECK(kf_source_keys_table(3, &once[0][0], tkey, tslot, mask) && mask == 7);
    // the invariant: mask + 1 a power of two >= 2 * count, every key found at its slot from its hash on before a free entry
    std::vector<int32_t> many;
    for (int z = -3; z < 4; ++z) for (int y = -2; y < 3; ++y) for (int x = 0; x < 9; ++x) { many.push_back(x * 37 - 100); many.push_back(y); many.push_back(z * 1000); }
    const uint32_t n = (uint32_t)(many.size() / 3);
    CHECK(kf_source_keys_table(n, many.data(), tkey, tslot, mask));
    CHECK(((uint64_t)mask + 1) >= 2ull * n && (((uint64_t)mask + 1) & mask) == 0 && tkey.size() == (size_t)mask + 1 && tslot.size() == tkey.size());
    for (uint32_t e = 0; e < n; ++e) {
      const unsigned long long key = kf_brick_key_pack(many[3 * e], many[3 * e + 1], many[3 * e + 2]);
      int64_t at = -1;
      for (uint32_t p = 0, h = kf_brick_key_hash(key, mask); p <= mask && tkey[h] != KF_BRICK_KEY_EMPTY; ++p, h = (h + 1u) & mask)
        if (tkey[h] == key) { at = (int64_t)tslot[h]; break; }
      CHECK(at == (int64_t)e);
    }
    many[3 * (n - 1)] = many[0]; many[3 * (n - 1) + 1] = many[1]; many[3 * (n - 1) + 2] = many[2];   // the last key names the first brick again
    CHECK(!kf_source_keys_table(n, many.data(), tkey, tslot, mask));
  }
  if (fails) { printf("%d checks FAILED\n", fails); return 1; }
  printf("map resample ok\n");
  return 0;
}
