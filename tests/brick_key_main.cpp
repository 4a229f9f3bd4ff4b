// A main of its own around csrc/brick_key.h, for a sanitizer run on the CPU (tests/test_brickstore_abi_cpu.py): reads world brick coordinates
// "x y z", one triple per line, and prints for each the packed key (hex), the three components unpacked from it and the key's place in a table of
// 2048 entries.  The first line printed is the word that marks a free table entry.
#include "brick_key.h"
#include <cinttypes>
#include <cstdio>

int main() {
  std::printf("%016" PRIx64 "\n", (uint64_t)KF_BRICK_KEY_EMPTY);
  long long x, y, z;
  int n = 0;
  while (std::scanf("%lld %lld %lld", &x, &y, &z) == 3) {
    if (!kf_brick_key_in_range(x) || !kf_brick_key_in_range(y) || !kf_brick_key_in_range(z)) { std::printf("out of range\n"); return 2; }
    const unsigned long long key = kf_brick_key_pack((int32_t)x, (int32_t)y, (int32_t)z);
    int32_t u[3];
    kf_brick_key_unpack(key, u);
    std::printf("%016" PRIx64 " %d %d %d %u\n", (uint64_t)key, u[0], u[1], u[2], kf_brick_key_hash(key, 2047u));
    ++n;
  }
  // the range test itself, at its four edges
  if (!kf_brick_key_in_range(KF_BRICK_KEY_MIN) || kf_brick_key_in_range((int64_t)KF_BRICK_KEY_MIN - 1) || !kf_brick_key_in_range((int64_t)KF_BRICK_KEY_MAX - 1) ||
      kf_brick_key_in_range(KF_BRICK_KEY_MAX)) { std::printf("range test wrong\n"); return 3; }
  std::printf("brick keys ok %d\n", n);
  return 0;
}
