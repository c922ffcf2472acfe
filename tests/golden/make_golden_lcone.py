#!/usr/bin/env python3
"""
Golden vectors of the lightcone sampling (reference cosmology.cube2lcone / cube2map), on the case tables of lcone_common:
inputs (cubes, angles) and the reference's outputs for 'nearest' and 'linear' radial x 'nearest' and 'linear' spatial
interpolation, ascending and descending sim_r, with and without roll, with angles and with angs=None, and cube2map itself.
'quadratic' is recorded under info_* for information only: the reference's branch is not the parabola through its cubes.

The reference's cosmology.py is imported by file path; astropy is absent, so astropy, astropy.units and astropy.constants
are MagicMock modules and astropy.cosmology.FlatLambdaCDM a plain empty class (cube2lcone / cube2map are numpy only).
TEST INFRASTRUCTURE ONLY, like make_golden.py; writes tests/golden/lcone.npz, arrays only, float64.

Usage:  python tests/golden/make_golden_lcone.py
"""
import importlib.util
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lcone_common as lc    # noqa: E402
from make_golden import REF as REF_DIR    # noqa: E402

REF = os.path.join(REF_DIR, 'cosmology.py')


def load_reference():
    sys.dont_write_bytecode = True
    for n in ('astropy', 'astropy.units', 'astropy.constants', 'astropy.cosmology'):
        sys.modules[n] = MagicMock(name=n)
    sys.modules['astropy.cosmology'].FlatLambdaCDM = type('FlatLambdaCDM', (), {})
    spec = importlib.util.spec_from_file_location('reference_cosmology', REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    sims, angs = lc.cubes(), lc.fixture_angs()
    out = {'sims': sims, 'angs': angs}
    for pinned in (True, False):
        for name, (order, ri, si, roll, sphere) in lc.fixture_cases(pinned).items():
            a = angs if sphere else None
            if order == 'map':
                got = ref.cube2map(sims[1], lc.R[2], lc.SIM_RES, angs=a, roll=roll, interp=si)
            else:
                got = ref.cube2lcone(sims, lc.SIM_R[order], lc.R, lc.SIM_RES, angs=a, rinterp=ri, interp=si, roll=roll)
            out[name] = np.asarray(got, dtype=np.float64)
    path = os.path.join(HERE, 'lcone.npz')
    np.savez_compressed(path, **out)
    print('wrote lcone.npz %.1f kB, %d arrays' % (os.path.getsize(path) / 1e3, len(out)))


if __name__ == '__main__':
    main()
