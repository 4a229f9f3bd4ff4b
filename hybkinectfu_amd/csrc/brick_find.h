// brick_find.h -- the brick store's read-only look-up (device), shared by brickstore.hip (restore, claim) and mapmesh.hip (the virtual window's resolve pass).
#pragma once
#include "kf_internal.h"
#include "brick_key.h"

// read-only: the slot of `key`, or KF_BRICK_NO_SLOT.  The probe ends at the first free entry: no entry is ever emptied in place (erase.hip rebuilds the whole table in launches of
// its own), so a key the table holds sits before it.
__device__ __forceinline__ unsigned store_find(const KfBrickStore& st, unsigned long long key) {
  unsigned h = kf_brick_key_hash(key, st.mask);
  for (unsigned p = 0; p <= st.mask; ++p, h = (h + 1u) & st.mask) {
    const unsigned long long k = st.tkey[h];
    if (k == key) { const unsigned slot = st.tslot[h]; return slot < st.max_bricks ? slot : KF_BRICK_NO_SLOT; }
    if (k == KF_BRICK_KEY_EMPTY) break;
  }
  return KF_BRICK_NO_SLOT;
}
