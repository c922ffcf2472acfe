#!/usr/bin/env python3
"""
Golden vectors of the sampler layer (reference sampler.py), on the separable potential and the case tables of hmc_common:
 (a) leapfrog outputs for tensor and ParamDict inputs with scalar, per-key and per-element eps, with and without cov_L, one
     complex key, and the `states` of one case;
 (b) an HMC chain (two keys, diagonal cov_L AND hess_L -- both passed, see below --, momenta supplied through pdist from
     recorded draws, np.random.seed fixed): prob, accept, U, x, p, K_start, H_end and the uniform draw of every move;
 (c) the same with a dHmax small enough that some moves are divergent;
 (d) eps after dual_averaging.
TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes tests/golden/hmc.npz, arrays only, float64 /
complex128.  Both Cholesky factors are passed because the reference derives hess_L from cov_L alone through a matrix diagonal
that has the wrong shape for a parameter of two or more dimensions.

The generator asserts what makes the recorded decisions robust: chain (b) holds an accepted and a rejected move, every
uniform draw is further than MARGIN from its probability, in (c) some but not all moves diverge and every energy change is
further than MARGIN from dHmax.

Usage:  python tests/golden/make_golden_hmc.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg     # noqa: E402
import hmc_common as hc      # noqa: E402


def load_sampler():
    mg.bootstrap_reference()
    for m in ('hmat', 'optim'):
        importlib.import_module('bayeslim.' + m)
    return importlib.import_module('bayeslim.sampler'), importlib.import_module('bayeslim.paramdict').ParamDict


def inputs(rng, keys):
    """per key: coefficients a, Cholesky factors (cov ~ 1 / sqrt(a), hess = 1 / cov), a start near the typical set"""
    a, cov, hess, x0 = {}, {}, {}, {}
    for k in keys:
        shape = hc.SHAPES[k]
        a[k] = rng.uniform(0.5, 2.0, shape)
        cov[k] = rng.uniform(0.8, 1.2, shape) / np.sqrt(a[k])
        hess[k] = 1.0 / cov[k]
        x0[k] = rng.normal(size=shape) / np.sqrt(a[k])
        if k == 'w':
            x0[k] = x0[k] + 1j * rng.normal(size=shape) / np.sqrt(a[k])
    return a, cov, hess, x0


def T(d):
    return {k: torch.as_tensor(v) for k, v in d.items()}


def gen_leapfrog(sm, ParamDict, rng, out):
    for name, (cont, keys, kind, with_cov) in hc.LEAP_CASES.items():
        a, cov, _, q0 = inputs(rng, keys)
        p0 = {k: rng.normal(size=hc.SHAPES[k]) + (1j * rng.normal(size=hc.SHAPES[k]) if k == 'w' else 0) for k in keys}
        if kind == 'scalar':
            eps = torch.tensor(hc.EPS_SCALAR)
        elif kind == 'key':
            eps = {k: np.array(0.03 + 0.02 * i) for i, k in enumerate(keys)}
        else:
            eps = {k: rng.uniform(0.02, 0.08, hc.SHAPES[k]) for k in keys}
        at = T(a)

        def dUdq(q, Ucache=None):
            if isinstance(q, torch.Tensor):
                U, g = hc.grad_U(at[keys[0]], q)
            else:
                U, g = 0, {}
                for k in q:
                    Uk, g[k] = hc.grad_U(at[k], q[k])
                    U = U + Uk
                g = ParamDict(g)
            if Ucache is not None:
                Ucache.append(U)
            return g

        if cont == 'tensor':
            k = keys[0]
            q, p = torch.as_tensor(q0[k]).clone(), torch.as_tensor(p0[k]).clone()
            e = eps if kind == 'scalar' else torch.as_tensor(eps[k])
            c = torch.as_tensor(cov[k]) if with_cov else None
        else:
            q, p = ParamDict(T(q0)).clone(), ParamDict(T(p0)).clone()
            e = eps if kind == 'scalar' else ParamDict(T(eps))
            c = ParamDict(T(cov)) if with_cov else {k: None for k in keys}     # (the reference cannot wrap None itself)
        states = [] if name == hc.LEAP_STATES else None
        sm.leapfrog(q, p, dUdq, e, hc.LEAP_N, cov_L=c, diag_mass=True, states=states)
        for k in keys:
            pre = 'leap_%s_' % name
            out[pre + 'q0_' + k], out[pre + 'p0_' + k], out[pre + 'a_' + k] = q0[k], p0[k], a[k]
            if kind != 'scalar':
                out[pre + 'eps_' + k] = eps[k]
            if with_cov:
                out[pre + 'cov_' + k] = cov[k]
            out[pre + 'q_' + k] = q if cont == 'tensor' else q[k]
            out[pre + 'p_' + k] = p if cont == 'tensor' else p[k]
            if states is not None:
                assert len(states) == hc.LEAP_N + 1
                out[pre + 'states_q_' + k] = torch.stack([s[0][k] for s in states])
                out[pre + 'states_p_' + k] = torch.stack([s[1][k] for s in states])
                out[pre + 'states_U'] = torch.stack([torch.as_tensor(float('nan') if s[2] is None else float(s[2])) for s in states])
        print('leapfrog %-12s done' % name)


def make_hmc(sm, ParamDict, a, cov, hess, x0, draws, dHmax, log, eps0=None):
    at = T(a)

    def potential(x):
        U, g = 0, {}
        for k in x:
            Uk, g[k] = hc.grad_U(at[k], x[k])
            U = U + Uk
        return U, ParamDict(g)

    class Recorder(sm.HMC):
        def K(self, p):
            out = super().K(p)
            log.setdefault('K', []).append(float(out))
            log.setdefault('p', []).append({k: mg.npy(p[k]).copy() for k in p})
            return out

        def is_divergent(self, H_start, H_end):
            out = bool(super().is_divergent(H_start, H_end))
            log.setdefault('H', []).append((float(H_start), float(H_end), out))
            return out

    count = {k: 0 for k in x0}

    def dist(k):
        def draw():
            count[k] += 1
            return torch.as_tensor(draws[k][count[k] - 1]).clone()
        return draw

    eps = ParamDict({k: torch.tensor(v) for k, v in (eps0 or hc.CHAIN['eps']).items()})
    return Recorder(potential, ParamDict(T(x0)), eps, cov_L=ParamDict(T(cov)), hess_L=ParamDict(T(hess)), diag_mass=True,
                    Nstep=hc.CHAIN['Nstep'], pdist={k: dist(k) for k in x0}, dHmax=dHmax)


def gen_chains(sm, ParamDict, rng, out):
    keys, steps = hc.CHAIN['keys'], hc.CHAIN['steps']
    a, cov, hess, x0 = inputs(rng, keys)
    draws = {k: rng.normal(size=(steps,) + hc.SHAPES[k]) for k in keys}
    for name, d in (('a', a), ('cov', cov), ('hess', hess), ('x0', x0), ('draws', draws)):
        for k in keys:
            out['chain_%s_%s' % (name, k)] = d[k]

    uniform, rand = [], np.random.rand

    def recording_rand():
        uniform.append(rand())
        return uniform[-1]

    np.random.rand = recording_rand
    try:
        for tag in ('b', 'c'):
            log = {}
            del uniform[:]
            np.random.seed(hc.CHAIN['seed'])
            dHmax = hc.CHAIN['dHmax_' + tag]
            s = make_hmc(sm, ParamDict, a, cov, hess, x0, draws, dHmax, log)
            rec = {n: [] for n in ('prob', 'accept', 'U', 'u')}
            xs = {k: [] for k in keys}
            for i in range(steps):
                n_u = len(uniform)
                accept, prob = s.step()
                s._acceptances.append(bool(accept))
                s.append_chain(s.x, U=s._U)
                rec['prob'].append(float(prob))
                rec['accept'].append(bool(accept))
                rec['U'].append(float(s._U))
                rec['u'].append(uniform[-1] if len(uniform) > n_u else np.nan)
                for k in keys:
                    xs[k].append(mg.npy(s.x[k]).copy())
            H = np.array([(h[0], h[1]) for h in log['H']])
            div = np.array([h[2] for h in log['H']])
            pre = 'chain_%s_' % tag
            out[pre + 'prob'], out[pre + 'accept'], out[pre + 'U'] = np.array(rec['prob']), np.array(rec['accept'], dtype=float), np.array(rec['U'])
            out[pre + 'u'], out[pre + 'div'] = np.array(rec['u']), div.astype(float)
            out[pre + 'K_start'], out[pre + 'H_end'], out[pre + 'H_start'] = np.array(log['K'][0::2]), H[:, 1], H[:, 0]
            for k in keys:
                out[pre + 'x_' + k] = np.stack(xs[k])
                out[pre + 'p_' + k] = np.stack([p[k] for p in log['p'][1::2]])
            dH = H[:, 1] - H[:, 0]
            print('chain %s: accept %s div %s\n  prob %s\n  u    %s\n  dH   %s' % (
                tag, rec['accept'], div.tolist(), np.round(rec['prob'], 4), np.round(rec['u'], 4), np.round(dH, 4)))
            ok = ~div
            assert np.all(np.abs(np.array(rec['u'])[ok] - np.array(rec['prob'])[ok]) > hc.MARGIN)
            assert np.all(np.abs(dH - dHmax) > hc.MARGIN)
            if tag == 'b':
                assert not div.any() and any(rec['accept']) and not all(rec['accept'])
            else:
                assert div.any() and not div.all() and div[1:].any()      # a restart with a chain to draw from
        # (d) dual averaging
        np.random.seed(hc.CHAIN['seed'])
        s = make_hmc(sm, ParamDict, a, cov, hess, x0, draws, hc.CHAIN['dHmax_b'], {}, eps0=hc.dual_eps0())
        s.dual_averaging(hc.CHAIN['Nadapt'])
        for k in keys:
            out['dual_eps_' + k] = s.eps[k]
            print('dual averaging: eps[%s] %.6g -> %.6g' % (k, hc.dual_eps0()[k], float(s.eps[k])))
            assert np.isfinite(float(s.eps[k]))
    finally:
        np.random.rand = rand


def gen():
    sm, ParamDict = load_sampler()
    rng = np.random.default_rng(917)
    out = {}
    gen_leapfrog(sm, ParamDict, rng, out)
    gen_chains(sm, ParamDict, rng, out)
    mg.save('hmc', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen()
