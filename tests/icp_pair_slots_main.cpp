// Stand-alone check of the pair rules of hybkinectfu_amd/csrc/icp_fold_slots.h: which 16-byte unit carries which two sums (icp_pair_of_sum,
// icp_pair_half_is_sum, icp_pair_byte_offset), which lane of the reduction stores it (icp_pair_store_lane, icp_pair_stored_by) and which lane of the fold
// polls which pair of which part (icp_fold_pair_lane).  Built with -fsanitize=address,undefined and run on the CPU by tests/test_icp_pair_slots_cpu.py.
// No device, no library: the header is all there is.
// The walk below is fold_partials_tagged's pair form: a polling lane (part, m) starts at w0 = part and steps by ICP_FOLD_BATCH * parts; in a batch it polls
// the units j < NS, unit j being pair m of the publisher w0 + j * parts -- or, where that publisher does not exist (the ragged last row), of w0 again, the
// value dropped; it adds both halves of every real unit to two chains and hands chain 0 to s_tot[part][2m] and chain 1 to s_tot[part][2m + 1] -- unless that
// half is the padding word.  For n_wg in 1 .. 1024 and 8 / 16 parts:
//   * every (publisher, sum) is added exactly once, by the part the single-word fold gives it to (w mod parts);
//   * the adds of a (part, sum) come in ascending publisher order;
//   * the padding half (word 27) reaches no total, and no total beyond the 27 sums is written;
//   * every polled unit lies inside the step's slot array, 16-byte aligned, and belongs to a publisher that exists.
#include "icp_fold_slots.h"
#include <stdio.h>
#include <vector>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static const int MAX_WG = 1024;                                            // KF_ICP_LOOP_MAX_WG: publishers a step's slot array has rows for
static const unsigned ARRAY_BYTES = MAX_WG * 32u * 8u;

static void check_fold(int n_wg, int parts) {
  const int threads = parts * 32;
  std::vector<int> adds((size_t)n_wg * 32, 0);                             // adds that reach a total, per (publisher, word)
  std::vector<int> written((size_t)parts * 32, 0);                         // s_tot[part][k] written
  int polling = 0;
  for (int t = 0; t < threads; ++t) {
    int part, m;
    if (!icp_fold_pair_lane(t, parts, part, m)) continue;
    ++polling;
    EXPECT(t < parts * 16 && part >= 0 && part < parts && m >= 0 && m < ICP_FOLD_PAIRS && part == t / 16);     // the first half of the workgroup, one DPP row per part
    std::vector<int> chain[2];
    int base = 0;
    for (int w0 = part; w0 < n_wg; w0 += ICP_FOLD_BATCH * parts, base += ICP_FOLD_BATCH * parts) {
      const int ns = icp_fold_batch_slots(n_wg, base, parts);
      for (int j = 0; j < ICP_FOLD_BATCH; ++j) {
        const int w = w0 + j * parts;
        if (w < n_wg) EXPECT(j < ns);                                      // no publisher beyond the polled units
        if (j >= ns) continue;
        const bool real = w < n_wg;
        const int polled = real ? w : w0;
        const unsigned off = icp_pair_byte_offset(polled, m);
        EXPECT(polled >= 0 && polled < n_wg && off % 16u == 0u && off + 16u <= ARRAY_BYTES);
        EXPECT(off == (unsigned)(polled * 32 + 2 * m) * 8u);               // the words 2m, 2m + 1 of the publisher's row, as single-word readers see them
        if (!real) continue;                                               // dropped: + 0.f
        chain[0].push_back(w); chain[1].push_back(w);
      }
    }
    for (int half = 0; half < 2; ++half) {
      if (!icp_pair_half_is_sum(m, half)) { EXPECT(m == ICP_FOLD_PAIRS - 1 && half == 1); continue; }      // the padding half: its chain goes nowhere
      const int k = 2 * m + half;
      EXPECT(k < ICP_SUMS && icp_pair_of_sum(k) == m);
      ++written[(size_t)part * 32 + k];
      int last = -1;
      for (size_t i = 0; i < chain[half].size(); ++i) {
        const int w = chain[half][i];
        EXPECT(w > last && w % parts == part);                             // ascending, and the part of the single-word fold
        last = w;
        ++adds[(size_t)w * 32 + k];
      }
    }
  }
  EXPECT(polling == ICP_FOLD_PAIRS * parts);
  for (int p = 0; p < parts; ++p)
    for (int k = 0; k < 32; ++k) EXPECT(written[(size_t)p * 32 + k] == (k < ICP_SUMS ? 1 : 0));
  for (int w = 0; w < n_wg; ++w)
    for (int k = 0; k < 32; ++k) EXPECT(adds[(size_t)w * 32 + k] == (k < ICP_SUMS ? 1 : 0));
}

// the publisher's side of the pair-store build variant (-DKF_ICP_STORE16): after the workgroup reduction lane 4 k + 3 holds sum k (k < 27) and every lane
// from 108 on holds 0.f
static void check_publish(int threads) {
  int stored[ICP_FOLD_PAIRS] = {0};
  for (int t = 0; t < threads; ++t) {
    const int m = icp_pair_stored_by(t);
    if (m < 0) continue;
    EXPECT(m < ICP_FOLD_PAIRS && t == icp_pair_store_lane(m));
    ++stored[m];
    const int lo = t - 4;                                                  // where the DPP shift (row_shr:4) reads
    EXPECT(lo >= 0 && (lo >> 4) == (t >> 4) && (lo >> 6) == (t >> 6));      // the same 16-lane row, hence the same wave
    EXPECT(lo == 4 * (2 * m) + 3);                                         // the holder of sum 2m
    if (icp_pair_half_is_sum(m, 1)) EXPECT(t == 4 * (2 * m + 1) + 3);      // the holder of sum 2m + 1
    else EXPECT(t >= ICP_SUMS * 4);                                        // the padding half: a lane that holds 0.f
  }
  for (int m = 0; m < ICP_FOLD_PAIRS; ++m) EXPECT(stored[m] == 1);
}

int main() {
  EXPECT(ICP_SUMS == 27 && ICP_FOLD_PAIRS == 14);
  EXPECT(icp_pair_half_is_sum(13, 0) && !icp_pair_half_is_sum(13, 1) && icp_pair_half_is_sum(12, 1));
  for (int parts : {8, 16})
    for (int n_wg = 1; n_wg <= MAX_WG; ++n_wg) check_fold(n_wg, parts);
  check_publish(256);
  check_publish(ICP_THREADS);
  if (fails) return 1;
  printf("icp pair slots ok\n");
  return 0;
}
