#!/usr/bin/env python3
"""
Golden vectors of the operator layer (reference hmat.py) for the case tables of tests/hmat_common.py: products, transposed
products and (N, 3) products of every tree with real and complex vectors, SolveMat(chol=True) and SolveHierMat (with and without
trans_solve) results, and two_loop_recursion with DiagMat, SparseMat, PartitionedMat and HierMat starting matrices.
TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes tests/golden/hmat.npz, float64 / complex128
arrays only.  Only what the reference computes correctly is recorded: every product is asserted against the dense float64
matrix that hmat_common assembles from the same arrays, and a case the reference cannot run is reported and left out.

Usage:  python tests/golden/make_golden_hmat.py
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
import hmat_common as hc     # noqa: E402


def load():
    mg.bootstrap_reference()
    sys.modules['bayeslim.optim'] = MagicMock()
    return importlib.import_module('bayeslim.hmat'), importlib.import_module('bayeslim.bfgs')


def solve_problem():
    rng = np.random.default_rng(5)
    n, n0 = 100, 40
    a = rng.normal(size=(n, n)) / np.sqrt(n)
    L = np.linalg.cholesky(a @ a.T + np.eye(n))
    return L, n0, rng.normal(size=n), rng.normal(size=n) + 1j * rng.normal(size=n)


def gen(hm, bf):
    T = torch.as_tensor
    out, left_out = {}, []

    def record(key, fn, want):
        try:
            got = fn().numpy()
        except Exception as e:                   # the reference cannot run this case
            left_out.append((key, repr(e)))
            return
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
        if got.shape != want.shape or not err < 1e-12:
            left_out.append((key, 'differs from the dense matrix by %.2e' % err))
            return
        out[key] = got

    for name, spec in hc.tree_specs().items():
        A = hc.dense(spec)
        op = hc.build(spec, hm, T)
        for tr in (False, True):
            M = A.T if tr else A
            for kind in hc.RHS_KINDS:
                x = hc.rhs(M.shape[1], kind)
                record('%s_%s_%s' % (name, 'T' if tr else 'N', kind), lambda: op.mat_vec_mul(T(x), transpose=tr), M @ x)

    L, n0, b, bc = solve_problem()
    for tag, v in (('real', b), ('complex', bc)):
        record('solvemat_chol_' + tag, lambda: hm.SolveMat(T(L), tri=True, lower=True, chol=True)(T(v)), np.linalg.solve(L @ L.T, v))
        for ts in (False, True):
            S = hm.SolveHierMat(T(L[:n0, :n0].copy()), T(L[n0:, n0:].copy()), A10=hm.DenseMat(T(L[n0:, :n0].copy())), lower=True,
                                trans_solve=ts)
            record('solvehier_%d_%s' % (ts, tag), lambda: S(T(v)), np.linalg.solve(L @ L.T if ts else L, v))

    s, y, vec, rho, specs = hc.tlr_problem()
    for kind in hc.TLR_KINDS:
        A = hc.dense(specs[kind])
        want = hc.two_loop_torch(T(vec), T(s), T(y), T(rho), lambda q: T(A) @ q).numpy()
        H0 = hc.build(specs[kind], hm, T)
        record('tlr_' + kind, lambda: bf.two_loop_recursion(T(vec), list(T(s)), list(T(y)), list(T(rho)), H0=H0), want)
    return out, left_out


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    out, left_out = gen(*load())
    for k, why in left_out:
        print('left out: %s (%s)' % (k, why))
    assert all(v.dtype in (np.float64, np.complex128) for v in out.values())
    path = os.path.join(HERE, 'hmat.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
