// Stand-alone check of the two counting rules of hybkinectfu_amd/csrc/icp_fold_slots.h: icp_fold_batch_slots -- how many tagged words a lane of the
// persistent loops' fold polls per batch -- and icp_level_geometry, the publishers per pyramid level that feed it.  Built with
// -fsanitize=address,undefined and run on the CPU by tests/test_icp_fold_slots_cpu.py.  No device, no library: the header is all there is.
// The walk below is fold_partials_tagged's: part p starts at w0 = p and steps by ICP_FOLD_BATCH * parts; in a batch it polls the slots j < NS, slot j being
// the publisher w0 + j * parts.  For n_wg in 1 .. 1024 and 8 / 16 parts:
//   * every compiled slot count is one of the ladder's, ascending, ICP_FOLD_BATCH the last, and the rule never leaves the ladder;
//   * no batch is given a slot count below its largest real slot count (no publisher is left out), nor a rung more than it needs;
//   * every (part, j) with a publisher is visited exactly once, in ascending w per part, and a slot without one lies in the ragged last row only.
#include "icp_fold_slots.h"
#include <stdio.h>
#include <vector>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static std::vector<int> ladder() {
  std::vector<int> l;
#define RUNG(n) l.push_back(n);
  ICP_FOLD_LADDER(RUNG)
#undef RUNG
  l.push_back(ICP_FOLD_BATCH);
  return l;
}

static void check(int n_wg, int parts, const std::vector<int>& rungs) {
  std::vector<int> visits((size_t)n_wg, 0);
  for (int part = 0; part < parts; ++part) {
    int base = 0, last_w = -1;
    for (int w0 = part; w0 < n_wg; w0 += ICP_FOLD_BATCH * parts, base += ICP_FOLD_BATCH * parts) {
      EXPECT(base == w0 - part);
      const int ns = icp_fold_batch_slots(n_wg, base, parts);
      // the real slots of this batch: the largest count over all parts is the first part's
      int rows = (n_wg - base + parts - 1) / parts;
      if (rows > ICP_FOLD_BATCH) rows = ICP_FOLD_BATCH;
      EXPECT(rows >= 1 && ns >= rows && ns <= ICP_FOLD_BATCH);
      bool on_ladder = false;
      for (size_t r = 0; r < rungs.size(); ++r) {
        if (rungs[r] == ns) on_ladder = true;
        if (rungs[r] >= rows && rungs[r] < ns) EXPECT(!"a lower rung would have done");
      }
      EXPECT(on_ladder);
      int real = 0;
      for (int j = 0; j < ICP_FOLD_BATCH; ++j) {
        const int w = w0 + j * parts;
        if (w >= n_wg) continue;
        EXPECT(j < ns);                                                   // a publisher beyond the polled slots would never be added
        if (j >= ns) continue;
        EXPECT(w > last_w);                                               // ascending per part: the order of the adds
        last_w = w;
        ++visits[(size_t)w];
        ++real;
      }
      EXPECT(real >= 1 && real >= rows - 1);                              // slots without a publisher: the ragged last row, no more
    }
  }
  for (int w = 0; w < n_wg; ++w) EXPECT(visits[(size_t)w] == 1);
}

static void level_counts(int cols, int rows, int want0, int want1, int want2) {
  const int want[3] = {want0, want1, want2};
  const int grid0 = (cols * rows + ICP_THREADS * ICP_PX - 1) / (ICP_THREADS * ICP_PX);
  for (int l = 0; l < 3; ++l) {
    int px_l, grid_l;
    icp_level_geometry((cols >> l) * (rows >> l), grid0, l, px_l, grid_l);
    EXPECT(grid_l == want[l] && px_l >= 1 && px_l <= ICP_PX && grid_l <= grid0);
    EXPECT((long long)grid_l * ICP_THREADS * px_l >= (long long)(cols >> l) * (rows >> l));      // every pixel has a lane
  }
}

int main() {
  const std::vector<int> rungs = ladder();
  for (size_t r = 0; r < rungs.size(); ++r) EXPECT(rungs[r] >= 1 && rungs[r] <= ICP_FOLD_BATCH && (r == 0 || rungs[r] > rungs[r - 1]));
  EXPECT(rungs.back() == ICP_FOLD_BATCH);
  for (int parts : {8, 16})
    for (int n_wg = 1; n_wg <= 1024; ++n_wg) check(n_wg, parts, rungs);
  // the shapes the ladder is cut for, at 16 parts: VGA's 38 / 150 / 200 publishers and the two batches of the SDF loop's 256
  EXPECT(icp_fold_batch_slots(38, 0, 16) == 3 && icp_fold_batch_slots(150, 0, 16) == 10 && icp_fold_batch_slots(200, 0, 16) == ICP_FOLD_BATCH);
  EXPECT(icp_fold_batch_slots(256, 0, 16) == ICP_FOLD_BATCH && icp_fold_batch_slots(256, ICP_FOLD_BATCH * 16, 16) == 3);
  // the edges: one publisher more than the rows below hold takes the next row
  EXPECT(icp_fold_batch_slots(48, 0, 16) == 3 && icp_fold_batch_slots(49, 0, 16) == 10 && icp_fold_batch_slots(160, 0, 16) == 10 &&
         icp_fold_batch_slots(161, 0, 16) == ICP_FOLD_BATCH);
  // publishers per level (icp_level_geometry) of VGA and of the images tests/test_gpu_icp_fold_shapes.py tracks
  level_counts(640, 480, 200, 150, 38);
  level_counts(256, 128, 22, 16, 4);
  level_counts(272, 128, 23, 17, 5);
  level_counts(656, 492, 211, 158, 40);
  if (fails) return 1;
  printf("icp fold slots ok\n");
  return 0;
}
