#!/usr/bin/env python3
"""
Golden vectors of the recycled sampler (reference sampler.py: RecycledHMC, StepSize, DynamicStepSize, pmask), on the separable
potential and the SHAPES of hmc_common with the complex key, momenta supplied through pdist from recorded draws, the host
generator seeded per chain (recycled_common.CHAINS).  Five chains of recycled_common.MOVES moves:
 (a) plain RecycledHMC;
 (b) a StepSize with a complex step on the complex key;
 (c) a DynamicStepSize whose update takes both branches, with an index on one key;
 (d) pmask with one real and one complex mask (and a mask of ones where recycled.RecycledHMC is given None: the reference
     cannot skip a key), set on the sampler after construction, as the reference's RecycledHMC takes none in its constructor;
     its K() multiplies the momentum by the mask in place at every step of the trajectory;
 (e) a dHmax small enough that some but not all moves diverge.
Per move: H_start, every H_i, every uniform draw, every accept, prob, x, _U, the chain length, and eps_mul for (c).
TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes tests/golden/recycled.npz, arrays only, float64 /
complex128.  Both Cholesky factors are passed, as in make_golden_hmc.py.

The generator asserts what makes the recordings robust: each chain holds an accepted and a rejected step, every uniform draw is
further than hmc_common.MARGIN from its probability AND every log-draw further than the float32 bound of recycled_common from its
energy difference, in (e) some but not all moves diverge and every energy change is further than both from dHmax.  It runs the
float64 restatement of recycled_common on the same inputs, asserts equal decisions, prints its largest discrepancy to the
reference (the constant RESTATEMENT of recycled_common) and asserts that the recordings stay within it.

Usage:  python tests/golden/make_golden_recycled.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg          # noqa: E402
import hmc_common as hc           # noqa: E402
import recycled_common as rc      # noqa: E402
from make_golden_hmc import load_sampler, inputs, T   # noqa: E402


def masks(rng):
    """{0, 1}-valued and sparse (the reference re-applies them at every step of a recycled trajectory, which drains energy: a dense
    mask leaves no rejected state): real on u, complex on w (each component masked on its own), ones on v"""
    m = {'u': (rng.uniform(size=hc.SHAPES['u']) < 0.97).astype(float), 'v': np.ones(hc.SHAPES['v'])}
    m['w'] = (rng.uniform(size=hc.SHAPES['w']) < 0.97) + 1j * (rng.uniform(size=hc.SHAPES['w']) < 0.97)
    m['w'][0], m['w'][1] = 1j, 1.0                  # at least one real and one imaginary part masked on their own
    return m


def make_sampler(sm, ParamDict, g, tag, log):
    a, x0, cov, hess, draws, eps, pmask, dyn, dHmax = rc.chain_setup(g, tag)
    at = T(a)

    def potential(x):
        U, gr = 0, {}
        for k in x:
            Uk, gr[k] = hc.grad_U(at[k], x[k])
            U = U + Uk
        return U, ParamDict(gr)

    class Recorder(sm.RecycledHMC):
        def is_divergent(self, H_start, H_end):
            out = bool(super().is_divergent(H_start, H_end))
            log.append((float(H_start), float(H_end), out))
            return out

    count = {k: 0 for k in x0}

    def dist(k):
        def draw():
            count[k] += 1
            return torch.as_tensor(draws[k][count[k] - 1]).clone()
        return draw

    e = {k: torch.as_tensor(v) for k, v in eps.items()}
    if tag == 'b':
        e = sm.StepSize(e)
    elif tag == 'c':
        e = sm.DynamicStepSize(e, **dyn)
    else:
        e = ParamDict(e)
    s = Recorder(potential, ParamDict(T(x0)), e, cov_L=ParamDict(T(cov)), hess_L=ParamDict(T(hess)), diag_mass=True,
                 Nstep=rc.NSTEP, dHmax=dHmax)
    s.pdist = {k: dist(k) for k in x0}
    if pmask is not None:
        s.pmask = ParamDict(T(pmask))
    return s


def gen():
    sm, ParamDict = load_sampler()
    rng = np.random.default_rng(2718)
    a, cov, hess, x0 = inputs(rng, rc.KEYS)
    draws = {k: rng.normal(size=(rc.MOVES,) + hc.SHAPES[k]) + (1j * rng.normal(size=(rc.MOVES,) + hc.SHAPES[k]) if k == 'w' else 0)
             for k in rc.KEYS}
    out = {}
    for name, d in (('a', a), ('cov', cov), ('hess', hess), ('x0', x0), ('draws', draws), ('mask', masks(rng))):
        for k in rc.KEYS:
            out['in_%s_%s' % (name, k)] = d[k]

    uniform, rand = [], np.random.rand

    def recording_rand():
        uniform.append(rand())
        return uniform[-1]

    np.random.rand = recording_rand
    worst = {}
    try:
        for tag in rc.TAGS:
            log = []
            np.random.seed(rc.CHAINS[tag]['seed'])
            s = make_sampler(sm, ParamDict, out, tag, log)
            recs = []
            for i in range(rc.MOVES):
                del log[:], uniform[:]
                n_acc = len(s._acceptances)
                accept, prob = s.step()
                recs.append(dict(H_start=log[0][0], H=[h[1] for h in log], u=list(uniform), div=log[-1][2], prob=float(prob),
                                 accept=[bool(x) for x in s._acceptances[n_acc:]], U=float(s._U), nchain=len(s.Uchain),
                                 x={k: mg.npy(s.x[k]).copy() for k in rc.KEYS},
                                 eps_mul={k: float(v) for k, v in s.eps.eps_mul.items()} if tag == 'c' else None))
                assert bool(accept) == (recs[-1]['accept'][-1] if not recs[-1]['div'] else False)
            acc, div, nchain = rc.decisions(recs)
            for name in ('H_start', 'prob', 'U'):
                out['%s_%s' % (tag, name)] = np.array([r[name] for r in recs])
            out[tag + '_H'], out[tag + '_u'] = rc.padded([r['H'] for r in recs]), rc.padded([r['u'] for r in recs])
            out[tag + '_accept'], out[tag + '_div'], out[tag + '_nchain'] = acc, div, nchain
            for k in rc.KEYS:
                out['%s_x_%s' % (tag, k)] = np.stack([r['x'][k] for r in recs])
            if tag == 'c':
                out['c_eps_mul'] = rc.eps_mul_of(recs)
            # what makes the record robust
            H, u, Hs = out[tag + '_H'], out[tag + '_u'], out[tag + '_H_start'][:, None]
            dH = H - Hs
            ok = ~np.isnan(u)
            prob = np.minimum(1.0, np.exp(-dH))
            b32 = rc.dH_bound(np.float32, float(np.nanmax(np.abs(H))))
            print('chain %s: accept %s\n  div %s  nchain %s  float32 bound %.3e' % (tag, acc.tolist(), div.tolist(), nchain.tolist(), b32))
            assert np.all(np.abs(u[ok] - prob[ok]) > hc.MARGIN)
            assert np.all(np.abs(np.log(u[ok]) - np.minimum(-dH[ok], 0.0)) > b32), np.abs(np.log(u[ok]) - np.minimum(-dH[ok], 0.0)).min()
            seen = ~np.isnan(dH)
            assert np.all(np.abs(dH[seen] - rc.CHAINS[tag]['dHmax']) > max(hc.MARGIN, b32))
            assert (acc[ok] == 1).any() and (acc[ok] == 0).any()
            if tag == 'e':
                assert div.any() and not div.all() and div[1:].any() and nchain[np.flatnonzero(div)[-1]] > 0
            else:
                assert not div.any()
            if tag == 'c':
                m = out['c_eps_mul']
                assert (np.diff(np.vstack([np.ones((1, 3)), m]), axis=0) < 0).any() and (np.diff(m, axis=0) > 0).any(), m
            # the restatement on the same inputs: same decisions, its discrepancy
            orecs = rc.run_oracle_chain(out, tag)
            worst[tag] = rc.chain_discrepancy(orecs, out, tag)
            assert np.array_equal(rc.padded([r['u'] for r in orecs]), u, equal_nan=True)
            if tag == 'c':
                assert np.array_equal(rc.eps_mul_of(orecs), out['c_eps_mul'])
            print('  restatement discrepancy %.3e' % worst[tag])
    finally:
        np.random.rand = rand
    top = max(worst, key=worst.get)
    print('RESTATEMENT = %.3g (chain %s); recycled_common holds %.3g' % (worst[top], top, rc.RESTATEMENT))
    mg.save('recycled', **out)
    assert worst[top] <= rc.RESTATEMENT, 'recycled_common.RESTATEMENT is below the measured discrepancy: record the new value'


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen()
