// map_reloc_main.cpp -- CPU check of the host side of relocalisation (host/reloc_search.hpp: reloc_points, reloc_lattice, reloc_rank), a program of its own:
// tests/test_map_reloc_abi_cpu.py builds it with AddressSanitizer + UBSan and runs it as a child process.  usage: map_reloc_main
#include "reloc_search.hpp"
#include <stdio.h>
#include <string.h>

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

int main() {
  // ---- points: valid vertices in row-major order, the subsample's indices, the median, the refusals
  {
    const uint32_t n = 1000;
    std::vector<float> v(4 * n);
    uint32_t valid = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const bool ok = i % 3 != 0;
      v[4 * i] = 0.01f * i; v[4 * i + 1] = -0.02f * i; v[4 * i + 2] = ok ? 1.f + 0.001f * ((i * 7) % 1000) : 0.f; v[4 * i + 3] = 1.f;
      valid += ok;
    }
    const float cell = 2.f / 64.f;
    std::vector<float> out(3 * n, -1.f);
    float med = -1.f;
    CHECK(reloc_points(v.data(), n, cell, n, out.data(), &med) == valid);
    CHECK(out[0] == (float)((double)v[4] / (double)cell) && out[2] == (float)((double)v[6] / (double)cell) && med > 1.f && med < 2.f);
    CHECK(out[3 * valid] == -1.f);                                 // nothing written past the count
    std::vector<float> few(3 * 100 + 1, -1.f);
    CHECK(reloc_points(v.data(), n, cell, 100, few.data(), nullptr) == 100u && few[300] == -1.f);
    // index floor(i * count / 100) of the valid list
    std::vector<uint32_t> list;
    for (uint32_t i = 0; i < n; ++i) if (i % 3 != 0) list.push_back(i);
    for (uint32_t i = 0; i < 100; ++i) CHECK(few[3 * i] == (float)((double)v[4 * list[(size_t)((uint64_t)i * valid / 100)]] / (double)cell));
    CHECK(reloc_points(nullptr, n, cell, 100, few.data(), &med) == 0u && med == 0.f);
    CHECK(reloc_points(v.data(), n, 0.f, 100, few.data(), nullptr) == 0u && reloc_points(v.data(), n, cell, 0, few.data(), nullptr) == 0u);
    CHECK(reloc_points(v.data(), 0, cell, 100, few.data(), &med) == 0u);
    std::vector<float> zeros(4 * 16, 0.f);
    CHECK(reloc_points(zeros.data(), 16, cell, 100, few.data(), &med) == 0u && med == 0.f);
  }
  // ---- lattice: the count, the order (translation outermost, jc fastest), the zero offset, the cap, the refusals
  {
    const double c[12] = {0, -1, 0, 10.5, 1, 0, 0, -3.25, 0, 0, 1, 7.0};
    const int32_t n[6] = {1, 0, 2, 1, 1, 0};
    const int64_t K = reloc_lattice(c, n, 4.0, 0.05, nullptr, 0);
    CHECK(K == 3 * 1 * 5 * 3 * 3 * 1);
    std::vector<double> P((size_t)K * 12 + 1, -7.0);
    CHECK(reloc_lattice(c, n, 4.0, 0.05, P.data(), K) == K && P[(size_t)K * 12] == -7.0);
    CHECK(P[3] == 10.5 - 4.0 && P[7] == -3.25 && P[11] == 7.0 - 8.0);                    // the first: every index at -n
    CHECK(P[12 + 3] == P[3] && P[12 + 11] == P[11] && P[12] != P[0]);                  // the second differs in the last rotation axis that moves (jb)
    const int64_t mid = K / 2;
    CHECK(memcmp(&P[(size_t)mid * 12], c, sizeof(c)) == 0);                            // the zero offset is the centre itself, bit for bit
    for (int64_t k = 0; k < K; ++k) {                                                  // every R is Rc times a rotation: orthonormal
      const double* R = &P[(size_t)k * 12];
      for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) {
        const double g = R[a] * R[b] + R[4 + a] * R[4 + b] + R[8 + a] * R[8 + b];
        CHECK(fabs(g - (a == b ? 1.0 : 0.0)) < 1e-14);
      }
    }
    std::vector<double> part(5 * 12 + 1, -7.0);
    CHECK(reloc_lattice(c, n, 4.0, 0.05, part.data(), 5) == K && part[60] == -7.0 && memcmp(part.data(), P.data(), 60 * sizeof(double)) == 0);
    const int32_t neg[6] = {1, 1, 1, -1, 1, 1}, big[6] = {5, 5, 5, 5, 5, 5}, ok20[6] = {7, 7, 7, 1, 1, 1};
    CHECK(reloc_lattice(c, neg, 1, 1, nullptr, 0) == -1 && reloc_lattice(c, big, 1, 1, nullptr, 0) == -1);   // 11^6 > 2^20
    CHECK(reloc_lattice(c, ok20, 1, 1, nullptr, 0) == 15 * 15 * 15 * 27 && reloc_lattice(nullptr, n, 1, 1, nullptr, 0) == -1 && reloc_lattice(c, nullptr, 1, 1, nullptr, 0) == -1);
  }
  // ---- rank: eligibility, the key, the ties, fewer eligible than asked for
  {
    kf_pose_score s[6] = {{100, 90, 5, 5, 50}, {100, 90, 5, 5, 40}, {10, 10, 0, 0, 1}, {200, 140, 30, 30, 9}, {100, 90, 5, 5, 40}, {100, 10, 80, 10, 7}};
    uint32_t best[8] = {99, 99, 99, 99, 99, 99, 99, 99};
    CHECK(reloc_rank(s, 6, 50, 3, best) == 5u);
    CHECK(best[0] == 3 && best[1] == 1 && best[2] == 4 && best[3] == 99);              // key 80 four times: sum_q 9 (index 3), 40 (index 1, then 4), 50 (index 0)
    CHECK(reloc_rank(s, 6, 50, 8, best) == 5u && best[3] == 0 && best[4] == 5 && best[5] == 99);
    CHECK(reloc_rank(s, 6, 1000, 8, best) == 0u && reloc_rank(nullptr, 6, 0, 8, best) == 0u && reloc_rank(s, 6, 0, 0, nullptr) == 6u);
  }
  const RelocParams d = hkf_reloc_defaults();
  CHECK(d.top == 16 && d.max_points == 4096 && d.level == -1 && d.n[0] == 2 && d.n[5] == 2 && d.has_guess == 0);
  printf(fails ? "map reloc FAILED\n" : "map reloc ok\n");
  return fails ? 1 : 0;
}
