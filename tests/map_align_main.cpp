// map_align_main.cpp -- CPU check of the host side of a map alignment (csrc/align_step.h: kf_align_solve6, kf_align_exp, kf_align_step_host; csrc/rigid_keys.h:
// kf_rigid_valid on the stepped transforms), a program of its own: tests/test_map_align_abi_cpu.py builds it with AddressSanitizer + UBSan and runs it as a
// child process.  usage: map_align_main
#include "align_step.h"
#include "rigid_keys.h"
#include <stdio.h>
#include <string.h>

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

// the 29 sums of rows J_k, e_k = J_k . xi_true + noise_k: a small deterministic generator (an LCG) gives well-spread rows
static unsigned long long lcg = 12345;
static double rnd() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0 - 0.5; }
static void sums_of(int n, const double xi[6], double noise, double s[KF_ALIGN_SUMS]) {
  memset(s, 0, sizeof(double) * KF_ALIGN_SUMS);
  for (int r = 0; r < n; ++r) {
    double J[6], e = noise * rnd();
    for (int a = 0; a < 6; ++a) { J[a] = (a < 3 ? 20.0 : 1.0) * rnd(); e += J[a] * xi[a]; }
    int k = 0;
    for (int a = 0; a < 6; ++a) for (int b = a; b < 6; ++b, ++k) s[k] += J[a] * J[b];
    for (int a = 0; a < 6; ++a) s[21 + a] += J[a] * e;
    s[27] += e * e; s[28] += 1.0;
  }
}

int main() {
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const double centre[3] = {32.0, 31.5, 30.0};
  // ---- the solve: rows without noise give the unknowns back
  {
    const double xi[6] = {0.01, -0.02, 0.03, 0.5, -0.25, 0.125};
    double s[KF_ALIGN_SUMS], got[6];
    sums_of(500, xi, 0.0, s);
    CHECK(kf_align_solve6(s, got));
    for (int a = 0; a < 6; ++a) CHECK(fabs(got[a] - xi[a]) < 1e-12);
  }
  // ---- the exponential: a quarter turn about z with a translation along z; small angles take the series
  {
    const double xi[6] = {0, 0, M_PI / 2, 0, 0, 2.0};
    double E[9], u[3];
    kf_align_exp(xi, E, u);
    CHECK(fabs(E[0]) < 1e-15 && fabs(E[1] + 1) < 1e-15 && fabs(E[3] - 1) < 1e-15 && fabs(E[4]) < 1e-15 && fabs(E[8] - 1) < 1e-15);
    CHECK(fabs(u[0]) < 1e-15 && fabs(u[1]) < 1e-15 && fabs(u[2] - 2.0) < 1e-15);
    const double tiny[6] = {1e-6, -2e-6, 3e-6, 1, 2, 3}, big[6] = {1.0000001e-4, 0, 0, 1, 2, 3}, below[6] = {0.9999999e-4, 0, 0, 1, 2, 3};
    double E2[9], u2[3];
    kf_align_exp(tiny, E, u);
    CHECK(fabs(E[1] + 3e-6) < 1e-11 && fabs(u[0] - (1 + 0.5 * (-3e-6 * 2 + -2e-6 * 3))) < 1e-11);
    kf_align_exp(big, E, u); kf_align_exp(below, E2, u2);      // the two branches agree where they meet
    for (int i = 0; i < 9; ++i) CHECK(fabs(E[i] - E2[i]) < 1e-10);
    for (int i = 0; i < 3; ++i) CHECK(fabs(u[i] - u2[i]) < 1e-10);
    const double zero[6] = {0, 0, 0, 0, 0, 0};
    kf_align_exp(zero, E, u);
    for (int i = 0; i < 9; ++i) CHECK(E[i] == (i % 4 == 0 ? 1.0 : 0.0));
  }
  // ---- the step: the update about the centre, the result still a transform after many steps
  {
    const double xi[6] = {0.02, 0.01, -0.03, 0.3, 0.2, -0.1};
    double s[KF_ALIGN_SUMS], xf[12], step[6];
    sums_of(400, xi, 1e-3, s);
    memcpy(xf, I, sizeof(xf));
    CHECK(kf_align_step_host(s, centre, xf, step) == 0 && kf_rigid_valid(xf));
    double E[9], u[3];
    kf_align_exp(step, E, u);
    for (int i = 0; i < 3; ++i) {                               // from the identity: R = E, t = centre - E centre + V v
      for (int j = 0; j < 3; ++j) CHECK(xf[4 * i + j] == E[3 * i + j]);
      const double t = (E[3 * i] * (0 - centre[0]) + E[3 * i + 1] * (0 - centre[1]) + E[3 * i + 2] * (0 - centre[2])) + centre[i] + u[i];
      CHECK(xf[4 * i + 3] == t);
    }
    for (int a = 0; a < 6; ++a) CHECK(fabs(step[a] - xi[a]) < 1e-3);
    for (int k = 0; k < 200; ++k) CHECK(kf_align_step_host(s, centre, xf, step) == 0);
    CHECK(kf_rigid_valid(xf));                                   // 201 rotations composed in fp64 stay orthonormal far inside the tolerance
  }
  // ---- refusals leave xf and step alone
  {
    double s[KF_ALIGN_SUMS] = {0}, xf[12], step[6] = {7, 7, 7, 7, 7, 7};
    memcpy(xf, I, sizeof(xf));
    CHECK(kf_align_step_host(s, centre, xf, step) != 0);        // a zero matrix
    const double xi[6] = {0.01, 0.01, 0.01, 0.1, 0.1, 0.1};
    sums_of(300, xi, 0.0, s);
    double z[KF_ALIGN_SUMS];
    memcpy(z, s, sizeof(z));
    int k = 0;
    for (int a = 0; a < 6; ++a) for (int b = a; b < 6; ++b, ++k) if (a == 2 || b == 2) z[k] = 0.0;      // row and column 2 zero: the third pivot is 0
    CHECK(kf_align_step_host(z, centre, xf, step) != 0);
    memcpy(z, s, sizeof(z)); z[0] = -z[0];
    CHECK(kf_align_step_host(z, centre, xf, step) != 0);        // a negative pivot
    memcpy(z, s, sizeof(z)); z[5] = NAN;
    CHECK(kf_align_step_host(z, centre, xf, step) != 0);
    memcpy(z, s, sizeof(z)); z[21] = INFINITY;
    CHECK(kf_align_step_host(z, centre, xf, step) != 0);
    CHECK(kf_align_step_host(nullptr, centre, xf, step) != 0 && kf_align_step_host(s, nullptr, xf, step) != 0 && kf_align_step_host(s, centre, nullptr, step) != 0 &&
          kf_align_step_host(s, centre, xf, nullptr) != 0);
    CHECK(memcmp(xf, I, sizeof(xf)) == 0);
    for (int a = 0; a < 6; ++a) CHECK(step[a] == 7.0);
    CHECK(kf_align_step_host(s, centre, xf, step) == 0);        // and the good sums still step
  }
  if (fails) { printf("%d checks FAILED\n", fails); return 1; }
  printf("map align ok\n");
  return 0;
}
