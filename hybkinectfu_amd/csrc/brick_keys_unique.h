// brick_keys_unique.h -- does a list of packed brick keys (brick_key.h) name every brick once?  Plain host C++: kf_write_brick_store asks before it
// launches (one import launch assumes that no two workgroups meet the same key), and the CPU test compiles this header into a program of its own
// (tests/map_file_main.cpp).  (The map file's codec has a test of its own: it needs the records in (z, y, x) order, which is not the packed keys' order.)
#pragma once
#include <stddef.h>
#include <algorithm>

// sorts `packed` in place; true when no two neighbours are equal afterwards (an empty list and a single key are unique)
static inline bool kf_brick_keys_unique(unsigned long long* packed, size_t n) {
  if (n < 2) return true;
  std::sort(packed, packed + n);
  return std::adjacent_find(packed, packed + n) == packed + n;
}
