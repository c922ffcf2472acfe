#!/usr/bin/env python3
"""
Golden vectors of the dense half of the optimiser layer (reference bfgs.py: BFGS, FactoredInvHessian, factor_pairs,
implicit_to_dense), on the tables of tests/bfgs_dense_common.py: BFGS.step trajectories (strong-Wolfe and fixed step, scalar and
dense H0, store_Hy) on the convex quadratic of make_golden_bfgs.py at N = 97, FactoredInvHessian in its rank-two and rank-one
forms built from the recorded lists of one trajectory, synthetic factor_pairs cases and implicit_to_dense for four starting
matrices.  TEST INFRASTRUCTURE ONLY, like make_golden_bfgs.py, whose loader of the reference it reuses; writes
tests/golden/bfgs_dense.npz, float64 arrays only (symmetric matrices as their upper triangle).

Usage:  python tests/golden/make_golden_bfgs_dense.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                      # noqa: E402
from make_golden_bfgs import load_bfgs        # noqa: E402
import bfgs_dense_common as dc                # noqa: E402


def gen(bf):
    out = {}
    N, cond = dc.DENSE['N'], dc.DENSE['cond']
    torch.manual_seed(0)
    a = torch.randn(N, int(cond * N), dtype=torch.float64)
    cov = (a @ a.T) / (cond * N)
    icov = torch.linalg.inv(cov)
    icov = 0.5 * (icov + icov.T)
    torch.manual_seed(100)
    out['dense_x0'] = torch.randn(N, dtype=torch.float64) * cov.diagonal().sqrt()
    out['dense_icov_triu'] = dc.triu(icov)
    g = {k: torch.as_tensor(mg.npy(v)) for k, v in out.items()}
    icov2, x0 = dc.dense_problem(g)
    assert torch.equal(icov2, icov)

    # trajectories
    for kind, h0 in dc.dense_cases():
        H0 = dc.dense_H0(icov, h0)
        H0_before = H0.clone()
        res, opt = dc.run_dense(bf.BFGS, icov, x0, H0, kind)
        assert torch.equal(H0, H0_before)
        for k, v in res.items():
            out['dense_%s_%s_%s' % (kind, h0, k)] = v
        print('trajectory %-6s %-6s losses %s exit %d func_evals %d n_iter %d pairs %d' % (
            kind, h0, ['%.6g' % v for v in res['losses'].tolist()], *res['ints'].tolist()))
    g = {k: torch.as_tensor(mg.npy(v)) for k, v in out.items()}
    assert int(g['dense_%s_%s_ints' % dc.FACTORED_RUN][3]) == dc.DENSE['max_iter'] * dc.DENSE['steps']

    # factored form from the recorded lists
    rng = np.random.default_rng(97)
    vec = torch.as_tensor(rng.normal(size=N))
    out['fact_vec'] = vec
    for kind in dc.FACTORED_KINDS:
        F = bf.FactoredInvHessian(**dc.factored_args(g, kind))
        key = 'fact_%s_' % kind
        out[key + 'u'], out[key + 'v'] = torch.stack(F.u), torch.stack(F.v)
        out[key + 'kept'] = np.array([len(F.u)])
        out[key + 'hvp'], out[key + 'lvp'] = F.hvp(vec), F.lvp(vec)
        out[key + 'H_triu'], out[key + 'L'] = dc.triu(F.to_dense(True)), F.to_dense(False)
        print('factored %-5s kept %d of %d pairs' % (kind, len(F.u), F.m))
        assert len(F.u) >= 2
    assert int(out['fact_rank2_kept'][0]) == dc.DENSE['max_iter'] * dc.DENSE['steps']
    Hfin = dc.from_triu(g['dense_%s_%s_H_triu' % dc.FACTORED_RUN], N)
    print('rank-two to_dense() against the final BFGS.H of the run: %.3e' % dc.rel(dc.from_triu(out['fact_rank2_H_triu'], N), Hfin))

    # factor_pairs on synthetic pairs
    spds = []
    for i, case in enumerate(dc.PAIR_CASES):
        s, y, gk, alpha, Hy = dc.pair_inputs(case)
        u, v, spd = bf.factor_pairs(s, y, gk, alpha, Hy, pos=case[2], rank2=case[1])
        out['pair_%d_u' % i], out['pair_%d_v' % i] = u, v
        spds.append(int(bool(spd)))
    out['pair_spd'] = np.array(spds)
    print('factor_pairs spd', spds)
    assert 0 in spds and 1 in spds

    # implicit_to_dense
    s, y = dc.factored_lists(g)[:2]
    for h0 in dc.ITD_H0S:
        out['itd_%s_H_triu' % h0] = dc.triu(bf.implicit_to_dense(dc.itd_H0(g, h0), s, y))
    out = {k: mg.npy(v).astype(np.float64) if mg.npy(v).dtype.kind == 'f' else mg.npy(v) for k, v in out.items()}
    mg.save('bfgs_dense', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen(load_bfgs())
