"""Compare two `bench.py --dump-outputs` directories array by array: largest |difference| relative to the largest |entry|.
usage: python tools/compare_dumps.py DIR_A DIR_B [bound]      exit status 1 when an array is missing, differs in shape or exceeds the bound"""
import os
import sys

import numpy as np


def main():
    a, b = sys.argv[1], sys.argv[2]
    bound = float(sys.argv[3]) if len(sys.argv) > 3 else None
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    worst, ok = 0.0, True
    for n in names:
        if not n.endswith(".npy"):
            continue
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{n}: only in one directory")
            ok = False
            continue
        x, y = np.load(pa), np.load(pb)
        if x.shape != y.shape:
            print(f"{n}: shapes {x.shape} and {y.shape}")
            ok = False
            continue
        scale = float(np.abs(x).max()) if x.size else 0.0
        diff = float(np.abs(x - y).max()) if x.size else 0.0
        # an all-zero array has no scale: equal arrays differ by 0, anything else counts as a full-size difference
        err = diff / scale if scale > 0 else (0.0 if diff == 0 else float("inf"))
        if not np.isfinite(err):
            ok = False
        worst = max(worst, err)
        print(f"{n}: shape {x.shape} largest |difference| / largest |entry| = {err:.3e}  bit-identical: {bool(np.array_equal(x, y))}")
    print(f"largest over all arrays: {worst:.3e}" + (f" (bound {bound:.3e})" if bound is not None else ""))
    if bound is not None and worst > bound:
        ok = False
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
