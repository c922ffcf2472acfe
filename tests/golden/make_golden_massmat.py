#!/usr/bin/env python3
"""
Golden vectors of the dense-mass sampler layer (reference sampler.py on the CPU, float64) for the quadratic potential
U = 1/2 sum_k q_k^T A_k q_k and the factors L = I + 0.3 tril(randn) / sqrt(n) of massmat_common:
 (a) sampler.leapfrog(..., cov_L=L, diag_mass=False) for a tensor;
 (b) the same for a ParamDict with one diagonal key, one dense real key and one dense complex key;
 (c) HMC.K of a momentum ParamDict;
 (d) a short HMC chain and (e) a short NUTS chain, momenta supplied through pdist from recorded arrays, np.random.seed fixed and
     np.random.rand wrapped so that every uniform draw is recorded: per move accept, prob, H_start, the proposal's H, the position,
     and for NUTS the tree depth and, per call of hoffman_uturn in the order of the calls, the two projections and the sums of the
     magnitudes of their terms.
The reference multiplies a complex momentum by the factor with torch's @, which wants one dtype: the complex key's real factor is
handed to the reference cast to complex128 (the same numbers; it then acts on the real and imaginary parts alike).
TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes tests/golden/massmat.npz, arrays only.

Usage:  python tests/golden/make_golden_massmat.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg          # noqa: E402
import make_golden_hmc as mgh     # noqa: E402
import massmat_common as mc       # noqa: E402

T = torch.as_tensor


def key_inputs(rng):
    """per key of mc.GOLDEN_KEYS: A, the factor (or the diagonal factor), x0"""
    A, L, x0 = {}, {}, {}
    for i, (k, kind, n) in enumerate(mc.GOLDEN_KEYS):
        A[k] = mc.spd(n, 100 + i)
        L[k] = rng.uniform(0.8, 1.2, n) if kind == 'diag' else mc.factor(n, 110 + i)
        x0[k] = rng.normal(size=n) + (1j * rng.normal(size=n) if kind == 'cdense' else 0)
    return A, L, x0


def ref_factor(L, kind):
    t = T(L)
    return t.to(torch.complex128) if kind == 'cdense' else t


def gen():
    sm, ParamDict = mgh.load_sampler()
    rng = np.random.default_rng(mc.GOLDEN_SEED)
    out = {}
    kinds = {k: kind for k, kind, _ in mc.GOLDEN_KEYS}
    eps = torch.tensor(mc.GOLDEN_EPS)                            # (the reference wraps a step size into a ParamDict: a tensor)
    dm = {k: kind == 'diag' for k, kind, _ in mc.GOLDEN_KEYS}

    # (a) a tensor
    n = mc.GOLDEN_TENSOR_N
    A, L = mc.spd(n, 90), mc.factor(n, 91)
    q0, p0 = rng.normal(size=n), rng.normal(size=n)
    q, p = T(q0).clone(), T(p0).clone()
    sm.leapfrog(q, p, lambda x, Ucache=None: T(A) @ x, eps, mc.GOLDEN_NSTEP, cov_L=T(L), diag_mass=False)
    out.update(t_A=A, t_L=L, t_q0=q0, t_p0=p0, t_q=q, t_p=p)

    # (b) a ParamDict
    A, L, x0 = key_inputs(rng)
    At = {k: T(A[k]) for k in A}
    cov = ParamDict({k: ref_factor(L[k], kinds[k]) for k in L})

    def grad(x):
        return ParamDict({k: (At[k].to(x[k].dtype) @ x[k]) for k in x})

    def potential(x):
        g = grad(x)
        return sum(0.5 * (x[k].conj() @ g[k]).real for k in x), g

    p0 = {k: rng.normal(size=v.shape) + (1j * rng.normal(size=v.shape) if np.iscomplexobj(v) else 0) for k, v in x0.items()}
    q, p = ParamDict({k: T(v).clone() for k, v in x0.items()}), ParamDict({k: T(v).clone() for k, v in p0.items()})
    sm.leapfrog(q, p, lambda x, Ucache=None: grad(x), eps, mc.GOLDEN_NSTEP, cov_L=cov, diag_mass=dm)
    for k in x0:
        out.update({'d_A_' + k: A[k], 'd_L_' + k: L[k], 'd_q0_' + k: x0[k], 'd_p0_' + k: p0[k], 'd_q_' + k: q[k], 'd_p_' + k: p[k]})

    # (c) - (e): the samplers
    steps = mc.GOLDEN_STEPS
    draws = {k: rng.normal(size=(2 * steps,) + v.shape) + (1j * rng.normal(size=(2 * steps,) + v.shape) if np.iscomplexobj(v) else 0)
             for k, v in x0.items()}
    for k in x0:
        out['draws_' + k] = draws[k]
    uniform, rand, uturn = [], np.random.rand, sm.hoffman_uturn
    angles = []

    def recording_rand():
        uniform.append(rand())
        return uniform[-1]

    def recording_uturn(q_minus, q_plus, p_minus, p_plus):
        lo = hi = slo = shi = 0.0
        for k in q_minus:
            span = (q_plus[k] - q_minus[k]).conj().ravel()
            lo += float((span @ p_minus[k].ravel()).real)
            hi += float((span @ p_plus[k].ravel()).real)
            slo += float((span.abs() * p_minus[k].ravel().abs()).sum())
            shi += float((span.abs() * p_plus[k].ravel().abs()).sum())
        angles.append((lo, hi, slo, shi))
        return uturn(q_minus, q_plus, p_minus, p_plus)

    def dist(k, count):
        def draw():
            count[k] += 1
            return T(draws[k][count[k] - 1]).clone()
        return draw

    np.random.rand, sm.hoffman_uturn = recording_rand, recording_uturn
    try:
        for tag, cls, kw in (('hmc', sm.HMC, dict(Nstep=mc.GOLDEN_NSTEP)), ('nuts', sm.NUTS, dict(max_tree_depth=mc.GOLDEN_DEPTH))):
            log = []

            class Recorder(cls):
                def is_divergent(self, H_start, H_end):
                    log.append((float(H_start), float(H_end)))
                    return super().is_divergent(H_start, H_end)

            count = {k: 0 for k in x0}
            np.random.seed(mc.GOLDEN_SEED)
            del uniform[:], angles[:]
            s = Recorder(potential, ParamDict({k: T(v).clone() for k, v in x0.items()}), ParamDict({k: eps.clone() for k in x0}),
                         cov_L=ParamDict({k: ref_factor(L[k], kinds[k]) for k in L}), diag_mass=dict(dm),
                         pdist={k: dist(k, count) for k in x0}, **kw)
            if tag == 'hmc':
                pk = ParamDict({k: T(p0[k]) for k in p0})
                out['K'] = float(s.K(pk))
                out['logdetM'] = float(s.logdetM)
            rec = {n_: [] for n_ in ('accept', 'prob', 'H_start', 'H_end', 'depth', 'u_last', 'nleaf')}
            xs = {k: [] for k in x0}
            for i in range(steps):
                del log[:]
                evals = s.fn_evals
                accept, prob = s.step()
                s._acceptances.append(bool(accept))
                s.append_chain(s.x, U=s._U)
                rec['accept'].append(float(bool(accept))), rec['prob'].append(float(prob)), rec['u_last'].append(uniform[-1])
                if tag == 'hmc':
                    rec['H_start'].append(log[-1][0]), rec['H_end'].append(log[-1][1]), rec['depth'].append(0.0)
                else:
                    rec['H_start'].append(log[0][0]), rec['H_end'].append(float(s._base_tree.q_prop_H))
                    leaves = s.fn_evals - evals - 1
                    rec['depth'].append(float(np.log2(leaves + 1)) if (leaves + 1) & leaves == 0 else -1.0)
                rec['nleaf'].append(float(s.fn_evals - evals - 1))
                for k in x0:
                    xs[k].append(mg.npy(s.x[k]).copy())
            for n_, v in rec.items():
                out['%s_%s' % (tag, n_)] = np.array(v)
            for k in x0:
                out['%s_x_%s' % (tag, k)] = np.stack(xs[k])
            if tag == 'nuts':
                out['nuts_angles'] = np.array(angles)
                out['nuts_leaf_H'] = np.array([h[1] for h in log])             # (of the last move)
            print(tag, {n_: np.round(v, 4).tolist() for n_, v in rec.items()})
    finally:
        np.random.rand, sm.hoffman_uturn = rand, uturn
    mg.save('massmat', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen()
