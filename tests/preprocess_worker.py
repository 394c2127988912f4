"""Worker of tests/test_gpu_preprocess_records.py::test_register_staged_kernels_write_the_same_bits (run as its own
process, not collected by pytest).  GSLM_PREPROCESS_STAGING is read once when libgslm.so loads, so the register-staged
kernels (k_preprocess<RAW, true>) can only be selected in a process of their own: the parent sets the variable to `reg`
in this process's environment.  Runs gslm_preprocess on the branch scene's (3, 3) and (2, 2) cases, layouts `leaf` and
`features`, both raw values, every prefix size and both views, and saves the parsed arrays to the .npz path given as
its one argument."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "gaussian-splatting-lm_amd"), HERE]

import numpy as np  # noqa: E402

WORKER_CASES = [(3, 3, False, 1.0), (2, 2, False, 1.0)]
WORKER_LAYOUTS = ("leaf", "features")


def key(case, P, b, raw, layout, field):
    return f"sh{case[0]}_{case[1]}/{P}/{b}/{int(raw)}/{layout}/{field}"


def main(path):
    import preprocess_layouts as pl
    assert os.environ.get("GSLM_PREPROCESS_STAGING") == "reg"
    out = {}
    for case in WORKER_CASES:
        for (P, b, raw, layout), r in pl.run_case(case, WORKER_LAYOUTS).items():
            for field, a in r.items():
                out[key(case, P, b, raw, layout, field)] = a
    np.savez(path, **out)
    print(f"saved {len(out)} arrays")


if __name__ == "__main__":
    main(sys.argv[1])
