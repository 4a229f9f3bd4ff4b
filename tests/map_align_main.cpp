// map_align_main.cpp -- CPU check of the host side of a map alignment (csrc/align_step.h: kf_align_solve6, kf_align_exp, kf_align_step_host, and the loop around
// them, kf_align_loop_turn, with every verdict and state transition on crafted sums; csrc/rigid_keys.h: kf_rigid_valid on the stepped transforms), a program of
// its own: tests/test_map_align_abi_cpu.py builds it with AddressSanitizer + UBSan and runs it as a
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
  // ---- the loop (kf_align_loop_turn): every verdict and every state transition, on crafted sums.  X0: a rigid start that is not the identity
  double X0[12];
  {
    const double xi[6] = {0.1, -0.2, 0.15, 3, -2, 1}, zero3[3] = {0, 0, 0};
    double E[9], u[3];
    kf_align_exp(xi, E, u);
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) X0[4 * i + j] = E[3 * i + j]; X0[4 * i + 3] = u[i]; }
    CHECK(kf_rigid_valid(X0));
    CHECK(kf_align_stop_valid(0.0, 0.0, centre, 1) && kf_align_stop_valid(1e-3, 1e-3, zero3, 0));
    const double bad[3] = {1, NAN, 3};
    CHECK(!kf_align_stop_valid(-1e-9, 0, centre, 1) && !kf_align_stop_valid(0, -1e-9, centre, 1) && !kf_align_stop_valid(NAN, 0, centre, 1) &&
          !kf_align_stop_valid(0, INFINITY, centre, 1) && !kf_align_stop_valid(0, 0, bad, 1));
  }
  const double zero6[6] = {0, 0, 0, 0, 0, 0};
  // count 0: FEW_PAIRS, nothing done, rms 0 -- also with min_pairs 0
  for (unsigned min_pairs = 0; min_pairs <= 100; min_pairs += 100) {
    KfAlignLoop L;
    double s[KF_ALIGN_SUMS] = {0};
    kf_align_loop_begin(L, X0);
    CHECK(!kf_align_loop_turn(L, s, centre, 25, min_pairs, 1e-9, 1e-9, true));
    CHECK(L.rep.verdict == KF_ALIGN_FEW_PAIRS && L.rep.iterations == 0 && L.rep.rms == 0.0);
    CHECK(memcmp(L.good, X0, sizeof(X0)) == 0 && memcmp(L.cur, X0, sizeof(X0)) == 0 && memcmp(L.rep.step, zero6, sizeof(zero6)) == 0);
  }
  // enough pairs, max_iter 0: ITER_LIMIT, the pose untouched, no step, the sums and their rms reported
  {
    const double xi[6] = {0.01, 0.02, -0.01, 0.2, 0.1, -0.3};
    KfAlignLoop L;
    double s[KF_ALIGN_SUMS];
    sums_of(300, xi, 0.01, s);
    kf_align_loop_begin(L, X0);
    CHECK(!kf_align_loop_turn(L, s, centre, 0, 300, 1e-9, 1e-9, true));
    CHECK(L.rep.verdict == KF_ALIGN_ITER_LIMIT && L.rep.iterations == 0 && L.rep.rms == sqrt(s[27] / 300.0) && L.rep.rms > 0.0);
    CHECK(memcmp(L.good, X0, sizeof(X0)) == 0 && memcmp(L.cur, X0, sizeof(X0)) == 0 && memcmp(L.rep.step, zero6, sizeof(zero6)) == 0);
    CHECK(memcmp(L.rep.sums, s, sizeof(s)) == 0);
    kf_align_loop_begin(L, X0);                                  // one pair short: FEW_PAIRS comes first
    CHECK(!kf_align_loop_turn(L, s, centre, 0, 301, 1e-9, 1e-9, true) && L.rep.verdict == KF_ALIGN_FEW_PAIRS && L.rep.rms == sqrt(s[27] / 300.0));
  }
  // a zero matrix with enough pairs: exactly SINGULAR, the pose the evaluated one
  for (int rigid = 0; rigid < 2; ++rigid) {
    KfAlignLoop L;
    double s[KF_ALIGN_SUMS] = {0};
    s[27] = 2.0; s[28] = 500.0;
    kf_align_loop_begin(L, X0);
    CHECK(!kf_align_loop_turn(L, s, centre, 25, 100, 1e-9, 1e-9, rigid != 0));
    CHECK(L.rep.verdict == KF_ALIGN_SINGULAR && L.rep.iterations == 0 && memcmp(L.rep.step, zero6, sizeof(zero6)) == 0);
    CHECK(memcmp(L.good, X0, sizeof(X0)) == 0 && memcmp(L.cur, X0, sizeof(X0)) == 0);
  }
  // a noise-free system: go on with iterations 1, the step the solve's, the pose stepped; then a step below eps: CONVERGED, the stepped pose returned
  {
    const double xi[6] = {0.02, 0.01, -0.03, 0.3, 0.2, -0.1}, small[6] = {1e-10, -2e-10, 1e-10, 3e-10, 1e-10, -1e-10};
    KfAlignLoop L;
    double s[KF_ALIGN_SUMS], want[12], solved[6], step[6];
    sums_of(500, xi, 0.0, s);
    memcpy(want, X0, sizeof(want));
    CHECK(kf_align_solve6(s, solved) && kf_align_step_host(s, centre, want, step) == 0);
    kf_align_loop_begin(L, X0);
    CHECK(kf_align_loop_turn(L, s, centre, 25, 100, 1e-9, 1e-9, true));
    CHECK(L.rep.iterations == 1 && memcmp(L.rep.step, solved, sizeof(solved)) == 0 && memcmp(L.cur, want, sizeof(want)) == 0);
    CHECK(memcmp(L.good, X0, sizeof(X0)) == 0 && memcmp(L.cur, X0, sizeof(X0)) != 0);
    sums_of(500, small, 0.0, s);
    CHECK(kf_align_step_host(s, centre, want, step) == 0);
    CHECK(!kf_align_loop_turn(L, s, centre, 25, 100, 1e-9, 1e-9, true));
    CHECK(L.rep.verdict == KF_ALIGN_CONVERGED && L.rep.iterations == 2 && memcmp(L.rep.step, step, sizeof(step)) == 0);
    CHECK(memcmp(L.good, want, sizeof(want)) == 0 && memcmp(L.cur, want, sizeof(want)) == 0 && memcmp(L.rep.sums, s, sizeof(s)) == 0);
  }
  // the eps floor: eps 0 converges on a step between 0 and the minima, and on neither side just above them
  {
    const double below[6] = {0.9 * KF_ALIGN_EPS_ROT_MIN, 0, 0, 0, 0.9 * KF_ALIGN_EPS_TRANS_MIN, 0};
    const double rot_above[6] = {1.1 * KF_ALIGN_EPS_ROT_MIN, 0, 0, 0, 0.9 * KF_ALIGN_EPS_TRANS_MIN, 0};
    const double trans_above[6] = {0.9 * KF_ALIGN_EPS_ROT_MIN, 0, 0, 0, 1.1 * KF_ALIGN_EPS_TRANS_MIN, 0};
    KfAlignLoop L;
    double s[KF_ALIGN_SUMS];
    sums_of(500, below, 0.0, s);
    kf_align_loop_begin(L, X0);
    CHECK(!kf_align_loop_turn(L, s, centre, 25, 100, 0.0, 0.0, true) && L.rep.verdict == KF_ALIGN_CONVERGED && L.rep.iterations == 1);
    CHECK(L.rep.step[0] > 0.0 && L.rep.step[0] < KF_ALIGN_EPS_ROT_MIN && L.rep.step[4] > 0.0 && L.rep.step[4] < KF_ALIGN_EPS_TRANS_MIN);
    sums_of(500, rot_above, 0.0, s);
    kf_align_loop_begin(L, X0);
    CHECK(kf_align_loop_turn(L, s, centre, 25, 100, 0.0, 0.0, true) && L.rep.iterations == 1);
    sums_of(500, trans_above, 0.0, s);
    kf_align_loop_begin(L, X0);
    CHECK(kf_align_loop_turn(L, s, centre, 25, 100, 0.0, 0.0, true) && L.rep.iterations == 1);
    sums_of(500, rot_above, 0.0, s);                             // an eps above the floor is the caller's
    kf_align_loop_begin(L, X0);
    CHECK(!kf_align_loop_turn(L, s, centre, 25, 100, 2.0 * KF_ALIGN_EPS_ROT_MIN, 0.0, true) && L.rep.verdict == KF_ALIGN_CONVERGED);
  }
  // FEW_PAIRS after one step: the pose evaluated before the step, iterations 1, that step, the second evaluation's sums
  {
    const double xi[6] = {0.02, 0.01, -0.03, 0.3, 0.2, -0.1};
    KfAlignLoop L;
    double s[KF_ALIGN_SUMS], few[KF_ALIGN_SUMS], first[6];
    sums_of(500, xi, 0.0, s);
    sums_of(99, xi, 0.5, few);
    kf_align_loop_begin(L, X0);
    CHECK(kf_align_loop_turn(L, s, centre, 25, 100, 1e-9, 1e-9, true));
    memcpy(first, L.rep.step, sizeof(first));
    CHECK(!kf_align_loop_turn(L, few, centre, 25, 100, 1e-9, 1e-9, true));
    CHECK(L.rep.verdict == KF_ALIGN_FEW_PAIRS && L.rep.iterations == 1 && memcmp(L.rep.step, first, sizeof(first)) == 0);
    CHECK(memcmp(L.good, X0, sizeof(X0)) == 0 && memcmp(L.cur, X0, sizeof(X0)) != 0);
    CHECK(memcmp(L.rep.sums, few, sizeof(few)) == 0 && L.rep.rms == sqrt(few[27] / 99.0));
  }
  // from a start that is not rigid: with require_rigid SINGULAR, iterations and step as they were; without it the loop goes on
  {
    const double xi[6] = {0.02, 0.01, -0.03, 0.3, 0.2, -0.1};
    double S[12], s[KF_ALIGN_SUMS], first[6];
    memcpy(S, X0, sizeof(S));
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) S[4 * i + j] *= 1.5;
    CHECK(!kf_rigid_valid(S));
    sums_of(500, xi, 0.0, s);
    KfAlignLoop L;
    kf_align_loop_begin(L, S);
    CHECK(!kf_align_loop_turn(L, s, centre, 25, 100, 1e-9, 1e-9, true));
    CHECK(L.rep.verdict == KF_ALIGN_SINGULAR && L.rep.iterations == 0 && memcmp(L.rep.step, zero6, sizeof(zero6)) == 0 && memcmp(L.good, S, sizeof(S)) == 0);
    kf_align_loop_begin(L, S);
    CHECK(kf_align_loop_turn(L, s, centre, 25, 100, 1e-9, 1e-9, false));
    CHECK(L.rep.iterations == 1 && memcmp(L.good, S, sizeof(S)) == 0 && !kf_rigid_valid(L.cur));
    memcpy(first, L.rep.step, sizeof(first));
    double at[12];
    memcpy(at, L.cur, sizeof(at));
    CHECK(!kf_align_loop_turn(L, s, centre, 25, 100, 1e-9, 1e-9, true));           // the same state, now asked to stay rigid
    CHECK(L.rep.verdict == KF_ALIGN_SINGULAR && L.rep.iterations == 1 && memcmp(L.rep.step, first, sizeof(first)) == 0 && memcmp(L.good, at, sizeof(at)) == 0);
  }
  if (fails) { printf("%d checks FAILED\n", fails); return 1; }
  printf("map align ok\n");
  return 0;
}
