#!/usr/bin/env python3
"""Generate tests/golden/ref_helpers.npz: what the REFERENCE's own __host__ __device__ helpers compute on the seeded inputs of
tests/test_oracle_vs_ref.py (REF_CASES x inputs_*), so that those tests also run where the reference's sources are absent.

Needs oracle/_ref/libkfref.so (oracle/Makefile builds it where the reference lies).   usage: python tools/make_ref_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["KF_REF_REGEN"] = "1"                 # reference_side() then returns the live arrays without comparing them with the old copy
import oracle_lib as O  # noqa: E402
import test_oracle_vs_ref as T  # noqa: E402


def main():
    if not O.have_ref():
        raise SystemExit("oracle/_ref/libkfref.so is not built: nothing to record")
    out = {}
    for name in T.REF_CASES:
        for k, a in T.reference_side(name, *getattr(T, "inputs_" + name)()).items():
            out[name + "/" + k] = a
    np.savez_compressed(T.GOLD, **out)
    print("%s: %d arrays, %d bytes" % (T.GOLD, len(out), os.path.getsize(T.GOLD)))


if __name__ == "__main__":
    main()
