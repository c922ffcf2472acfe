#!/usr/bin/env python3
"""
Golden vectors of the two log-priors this package evaluates on the fused prior kernel: the reference's LogLaplacePrior and
LogTaperedUniformPrior on the cases of prior_common.golden_cases -- every side, one or both bounds, alpha 1, 10 and 1e4,
scalar and full operands, a few hundred elements each, float64 -- with the value and its autograd gradient.  Only cases
where the reference is finite are recorded (a case that is not stops the script).

The reference is imported as make_golden.py does.  TEST INFRASTRUCTURE ONLY; writes tests/golden/prior.npz, arrays only.

Usage:  python tests/golden/make_golden_prior.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import prior_common as pc    # noqa: E402
from make_golden import bootstrap_reference, save    # noqa: E402


def main():
    bootstrap_reference()
    optim = importlib.import_module('bayeslim.optim')
    ten = lambda a: None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float64))
    out = {}
    for name, cls, kw, x in pc.golden_cases():
        if cls == 'laplace':
            prior = optim.LogLaplacePrior(ten(kw['mean']), ten(kw['scale']), side=kw['side'], density=kw['density'])
        else:
            prior = optim.LogTaperedUniformPrior(ten(kw['lower_bound']), ten(kw['upper_bound']), kind=kw['kind'],
                                                 alpha=torch.as_tensor(kw['alpha'], dtype=torch.float64))
        p = torch.as_tensor(x).clone().requires_grad_(True)
        val = prior(p)
        val.backward()
        assert torch.isfinite(val) and torch.isfinite(p.grad).all(), name
        out[name + '_x'], out[name + '_value'], out[name + '_grad'] = x, val.detach().numpy(), p.grad.numpy()
    save('prior', **out)


if __name__ == '__main__':
    main()
