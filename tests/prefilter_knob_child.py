"""Child process of tests/test_gpu_prefilter.py::test_static_knobs_in_fresh_processes: the VT_PF_* knobs that the library reads once
per process are set in this process's environment by the parent.  Runs KNOB_SHAPES through vt_prefilter_inplace against the float64
recursion, prints one line per case and exits with 1 when a case misses the bound.  Not a test module."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import prefilter_model as pm                      # noqa: E402
import test_gpu_prefilter as gp                   # noqa: E402


def main():
    env = {k: v for k, v in os.environ.items() if k.startswith('VT_PF_')}
    status = 0
    for shape in gp.KNOB_SHAPES:
        for kind in gp.KINDS:
            vol, c64 = gp.make_vol(shape, kind), gp.reference(shape, kind)
            got = gp.run_dense(vol)
            r_gpu = float(np.abs(got - c64).max()) / pm.unit(c64)
            ok = r_gpu <= gp.F64_FACTOR * gp.R_REF
            print(f'PFR knob {env} {shape} {kind} [{gp.form_names(pm.route_dense(shape, env=env))}] r_gpu={r_gpu:.2f} {"ok" if ok else "MISS"}')
            if not ok:
                status = 1
    return status


if __name__ == '__main__':
    sys.exit(main())
