"""
Helper launched by tests/test_gpu_sparse.py::test_predict_fallback_route_in_a_child with MFGM_SPARSE_PREDICT_V=0 in its environment (the
switch is read once per process): mfgm_sparse_predict and, for d > 8, mfgm_sparse_predict_kl at every even d on the cases of
tests/np_sparse.py, which k_sparse_predict<D2P> then serves instead of k_sparse_predict_v<NJ>.  The outputs go to the .npz file named
on the command line; the parent holds them to the reference.  Exit code 0 = every call returned 0 and two launches agreed bit for bit.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vidp_amd  # noqa: E402
from tests.test_gpu_sparse import PREDICT_CASES, Dev, case, plan_of  # noqa: E402


def main():
    assert os.environ.get("MFGM_SPARSE_PREDICT_V") == "0"
    vidp_amd._lib.load()
    out = {}
    for d in range(2, 33, 2):
        for M1, ends in PREDICT_CASES:
            cs = case(d, M1, ends)
            D = Dev(vidp_amd, cs)
            key = f"{d}_{M1}_{int(ends)}"
            for kl in (False, True) if d > 8 else (False,):
                plan = plan_of(vidp_amd, cs.M, d) if kl else None
                rc, fmu, fvar, tr, mh = D.predict(plan)
                again = D.predict(plan)
                assert rc == 0 and again[0] == 0, (key, rc)
                assert np.array_equal(fmu, again[1]) and np.array_equal(fvar, again[2]) and tr == again[3] and mh == again[4], key
                out[f"fmu_{key}_{int(kl)}"], out[f"fvar_{key}_{int(kl)}"] = fmu, fvar
                if kl:
                    out[f"kl_{key}"] = np.array([tr, mh])
    np.savez(sys.argv[1], **out)
    print("fallback route outputs written", len(out))


if __name__ == "__main__":
    main()
