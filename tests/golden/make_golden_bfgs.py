#!/usr/bin/env python3
"""
Golden vectors of the optimiser layer (reference bfgs.py): two_loop_recursion for the histories of lbfgs_common (scalar and
diagonal H0, one complex case), cubic_interpolate on the argument table of lbfgs_common, strong_wolfe on its two objectives,
and two full LBFGS trajectories (strong-Wolfe and fixed step) on a convex quadratic built as the reference's own test
problem (tests/test_bfgs.py::setup_NormalProb: cov = a a^T / (cond N), loss = x^T cov^-1 x / 2) in plain torch.
TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes tests/golden/bfgs.npz, arrays only,
everything float64 / complex128 (the inverse covariance as its upper triangle).

The reference's bfgs.py imports optim, hmat, paramdict and utils: hmat (DiagMat carries the starting matrix of LBFGS),
paramdict and utils are the reference's own, optim is satisfied with a mock (nothing here reaches it).

Usage:  python tests/golden/make_golden_bfgs.py
"""
import importlib
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg     # noqa: E402
import lbfgs_common as lc    # noqa: E402


def load_bfgs():
    mg.bootstrap_reference()
    sys.modules['bayeslim.optim'] = MagicMock()
    importlib.import_module('bayeslim.hmat')
    return importlib.import_module('bayeslim.bfgs')


def history(rng, N, m, cplx=False):
    """m pairs with s_i . y_i > 0: y = A s for a fixed positive diagonal plus a small symmetric low-rank part"""
    def rnd(*shape):
        x = rng.normal(size=shape)
        return x + 1j * rng.normal(size=shape) if cplx else x
    u = rng.uniform(0.5, 2.0, N)
    w = rng.normal(size=(N, 2)) / np.sqrt(N)
    s = rnd(m, N)
    y = s * u + 0.3 * (s @ w) @ w.T
    assert all((np.vdot(s[i], y[i])).real > 0 for i in range(m))
    return torch.as_tensor(s), torch.as_tensor(y), torch.as_tensor(rnd(N))


def gen(bf):
    rng = np.random.default_rng(411)
    out = {}
    for N in lc.TLR_NS:
        out['tlr_%d_diag' % N] = torch.as_tensor(rng.uniform(0.2, 3.0, N))
        for m in lc.TLR_MS:
            s, y, vec = history(rng, N, m)
            rho = [1.0 / (y[i] @ s[i]) for i in range(m)]
            key = 'tlr_%d_%d' % (N, m)
            out[key + '_s'], out[key + '_y'], out[key + '_vec'] = s, y, vec
            out[key + '_rho'] = torch.stack(rho)
            for kind in lc.TLR_KINDS:
                H0 = torch.tensor(lc.TLR_SCALAR, dtype=torch.float64) if kind == 'scalar' else out['tlr_%d_diag' % N]
                out[key + '_%s_out' % kind] = bf.two_loop_recursion(vec, list(s), list(y), rho, H0)
    N, m = lc.TLR_COMPLEX['N'], lc.TLR_COMPLEX['m']
    s, y, vec = history(rng, N, m, cplx=True)
    rho = [1.0 / (y[i].conj() @ s[i]).real for i in range(m)]
    out['tlrc_s'], out['tlrc_y'], out['tlrc_vec'], out['tlrc_rho'] = s, y, vec, torch.stack(rho)
    out['tlrc_diag'] = torch.as_tensor(rng.uniform(0.2, 3.0, N))
    out['tlrc_out'] = bf.two_loop_recursion(vec, list(s), list(y), rho, out['tlrc_diag'])
    assert out['tlrc_out'].is_complex()

    # cubic_interpolate
    res = []
    for row in lc.CUBIC_ARGS:
        a = [torch.tensor(v, dtype=torch.float64) for v in row[:6]]
        bounds = None if np.isnan(row[6]) else (row[6], row[7])
        res.append(float(bf.cubic_interpolate(*a, bounds=bounds)))
    out['cubic_out'] = np.array(res)

    # strong_wolfe
    for name in ('newton', 'quartic'):
        f, x0, p, alpha0, c2 = lc.wolfe_objective(name)
        loss, grad = f(x0)
        gp = grad @ p
        f_new, g_new, alpha, n = bf.strong_wolfe(lc.wolfe_obj_func(f), x0, alpha0, p, float(loss), grad, gp, c1=1e-4, c2=c2,
                                                 tolerance_change=1e-9, max_ls=25)
        out['wolfe_%s_scalars' % name] = np.array([float(f_new), float(alpha), float(n)])
        out['wolfe_%s_grad' % name] = g_new
        print('strong_wolfe %-8s f %.6g alpha %.6g evaluations %d' % (name, float(f_new), float(alpha), n))
    assert out['wolfe_newton_scalars'][2] == 1 and out['wolfe_quartic_scalars'][2] == 5

    # trajectories
    N, cond = lc.TRAJ['N'], lc.TRAJ['cond']
    torch.manual_seed(0)
    a = torch.randn(N, int(cond * N), dtype=torch.float64)
    cov = (a @ a.T) / (cond * N)
    icov = torch.linalg.inv(cov)
    icov = 0.5 * (icov + icov.T)
    torch.manual_seed(100)
    out['traj_x0'] = torch.randn(N, dtype=torch.float64) * cov.diagonal().sqrt()
    iu = torch.triu_indices(N, N)
    out['traj_icov_triu'] = icov[iu[0], iu[1]]
    g = {k: torch.as_tensor(mg.npy(v)) for k, v in out.items()}
    icov2, x0, H0 = lc.traj_problem(g)
    assert torch.equal(icov2, icov)
    for kind in lc.TRAJ_KINDS:
        res, opt = lc.run_trajectory(bf.LBFGS, icov2, x0, H0, kind)
        for k, v in res.items():
            out['traj_%s_%s' % (kind, k)] = v
        print('trajectory %-6s losses %s exit %d func_evals %d n_iter %d pairs %d' % (
            kind, ['%.6g' % v for v in res['losses'].tolist()], *res['ints'].tolist()))
        assert len(opt._s) == lc.TRAJ['history_size']
    mg.save('bfgs', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen(load_bfgs())
