#!/usr/bin/env python3
"""Compare two ``bench.py --dump-outputs`` folders file by file.

    python tools/compare_dumps.py DIR_A DIR_B [--atol 0]

Prints, per ``.npy`` file of DIR_A, how many rows (images) differ from DIR_B's file of the
same name by more than ``--atol`` and the largest difference; exits 1 if any do or a file is
missing.  Two runs with the same arguments have identical inputs, so every difference is
the computation's (docs/replica_nondeterminism.md)."""
import argparse
import os
import sys

import numpy as np


def compare(dir_a, dir_b, atol=0.0):
    """[(name, rows differing, rows, max |a - b|)], None for the counts of a missing or reshaped file."""
    out = []
    for name in sorted(f for f in os.listdir(dir_a) if f.endswith(".npy")):
        a = np.load(os.path.join(dir_a, name))
        path_b = os.path.join(dir_b, name)
        b = np.load(path_b) if os.path.exists(path_b) else None
        if b is None or a.shape != b.shape:
            out.append((name, None, a.shape[0], None))
            continue
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)).reshape(a.shape[0], -1).max(axis=1)
        out.append((name, int((d > atol).sum()), a.shape[0], float(d.max()) if d.size else 0.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--atol", type=float, default=0.0)
    a = ap.parse_args()
    bad = False
    for name, n, rows, mx in compare(a.dir_a, a.dir_b, a.atol):
        if n is None:
            print(f"{name}: missing in {a.dir_b} or of another shape")
            bad = True
        else:
            print(f"{name}: {n} of {rows} rows differ, max |d| {mx:.3g}")
            bad = bad or n > 0
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
