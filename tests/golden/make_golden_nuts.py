#!/usr/bin/env python3
"""
Golden vectors of the No-U-Turn sampler (reference sampler.NUTS, on the CPU) on the separable potential, the shapes and the
chain inputs (a, x0, cov, hess; two keys, 339 elements) of hmc_common / tests/golden/hmc.npz: the three chains of
nuts_common.CHAINS, STEPS moves each, momenta supplied through pdist from recorded draws, np.random.seed fixed and np.random.rand
wrapped so that every uniform draw is recorded:
 (a) biased progressive sampling, sampled directions;
 (b) uniform progressive sampling, forward only, track_states;
 (c) a dHmax small enough that moves diverge.
Per move: accept, prob, U, x, the proposal's H, H_start, the tree depth reached, fn_evals, whether it restarted from the chain,
the direction of every doubling, the uniform draws, and per leaf in the order they were built K (with logdetM), H and the two
angles of hoffman_uturn between the base tree's far edge and the leaf (computed here with the reference's expression).  Chain (b)
also records the number of tracked states.  TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes
tests/golden/nuts.npz, arrays only, float64.

The generator asserts what makes the record decisive: a move that ends by turning before max_tree_depth and one that reaches it,
both directions, both outcomes of a merge draw, an accepted and a rejected move; in (c) a restart from the chain and a divergence
at a tree depth of two or more, after which the move continues; every uniform draw further than MARGIN from the probability it is
compared with, every leaf's energy change further than MARGIN from dHmax, every angle larger than ANGLE_MARGIN times the sum of
the magnitudes of its terms.

Usage:  python tests/golden/make_golden_nuts.py
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
import hmc_common as hc           # noqa: E402
import nuts_common as nc          # noqa: E402


def make_nuts(sm, ParamDict, a, cov, hess, x0, draws, cfg, log):
    at = mgh.T(a)

    def potential(x):
        U, g = 0, {}
        for k in x:
            Uk, g[k] = hc.grad_U(at[k], x[k])
            U = U + Uk
        return U, ParamDict(g)

    class Recorder(sm.NUTS):
        _level, _in_leaf = 0, False

        def K(self, p):
            out = super().K(p)
            if self._in_leaf:
                log['leaf_K'].append(float(out))
            return out

        def _build_basetree(self, *args, **kwargs):
            self._in_leaf = True
            try:
                return super()._build_basetree(*args, **kwargs)
            finally:
                self._in_leaf = False

        def merge_trees(self, old_tree, new_tree, new_tree_right):
            d = new_tree.weight - (old_tree.weight if self.biased else sm._logaddexp(old_tree.weight, new_tree.weight))
            log['merge_p'].append(float(d.exp().clamp(max=1.0)))
            return super().merge_trees(old_tree, new_tree, new_tree_right)

        def build_tree(self, q, p, direction, tree_depth, H_start, dUdq0=None, base_tree=None):
            top = self._level == 0
            self._level += 1
            try:
                t = super().build_tree(q, p, direction, tree_depth, H_start, dUdq0=dUdq0, base_tree=base_tree)
            finally:
                self._level -= 1
            if tree_depth == 0:
                far_q, far_p = (base_tree.q_left, base_tree.p_left) if direction > 0 else (base_tree.q_right, base_tree.p_right)
                N = lambda d: {k: mg.npy(d[k]) for k in d}
                (minus, plus), scale = nc.angles(N(far_q), N(far_p), N(t.q_left), N(t.p_left), direction)
                # the reference's own expression, on its tensors
                lo = (far_q, t.q_right, far_p, t.p_right) if direction > 0 else (t.q_left, far_q, t.p_left, far_p)
                ref_minus = sum(float(((lo[1][k] - lo[0][k]).conj().ravel() @ lo[2][k].ravel()).real) for k in far_q)
                ref_plus = sum(float(((lo[1][k] - lo[0][k]).conj().ravel() @ lo[3][k].ravel()).real) for k in far_q)
                assert sm.hoffman_uturn(*lo) == ((ref_minus < 0) or (ref_plus < 0))
                log['leaf_minus'].append(ref_minus), log['leaf_plus'].append(ref_plus)
                log['angle_scale'] += list(scale)
                log['leaf_H'].append(float(t.q_prop_H))
            if top:
                log['H_start'] = float(H_start)
                log['doublings'].append((float(direction), int(tree_depth), bool(t.diverging), bool(t.turning)))
            return t

    count = {k: 0 for k in x0}

    def dist(k):
        def draw():
            count[k] += 1
            return torch.as_tensor(draws[k][count[k] - 1]).clone()
        return draw

    eps = ParamDict({k: torch.tensor(cfg['eps']) for k in x0})
    return Recorder(potential, ParamDict(mgh.T(x0)), eps, cov_L=ParamDict(mgh.T(cov)), hess_L=ParamDict(mgh.T(hess)), diag_mass=True,
                    pdist={k: dist(k) for k in x0}, dHmax=cfg['dHmax'], max_tree_depth=cfg['max_tree_depth'], biased=cfg['biased'],
                    track_states=cfg['track_states'], sample_direction=cfg['sample_direction'])


def draw_probabilities(cfg, doublings, merge_p, restart, prob):
    """the probability every uniform draw of a move was compared with, in the order of the draws"""
    ps, merges = [], list(merge_p)
    for direction, depth, diverging, turning in doublings:
        if cfg['sample_direction']:
            ps.append(0.5)
        inner = 2 ** depth - 1
        ps += merges[:inner]
        del merges[:inner]
        if not (diverging or turning):
            ps.append(merges.pop(0))
    assert not merges
    return ps + ([] if restart else [prob])


def run_chain(sm, ParamDict, tag, a, cov, hess, x0, draws, uniform, verbose=True):
    """the recorded arrays of one chain and the facts the generator asserts on"""
    cfg = nc.CHAINS[tag]
    log = {}
    del uniform[:]
    np.random.seed(cfg['seed'])
    s = make_nuts(sm, ParamDict, a, cov, hess, x0, draws, cfg, log)
    rec = {n: [] for n in nc.PER_MOVE + nc.PER_LEAF + ('dirs', 'u', 'nstates')}
    xs = {k: [] for k in nc.KEYS}
    facts = dict(turned_early=False, full_depth=False, dirs=set(), merges=set(), accepts=set(), restart=False, late_div=False, ok=True)
    for i in range(nc.STEPS):
        log.update(leaf_K=[], leaf_H=[], leaf_minus=[], leaf_plus=[], angle_scale=[], merge_p=[], doublings=[])
        n_u, evals = len(uniform), s.fn_evals
        s._base_tree = None
        accept, prob = s.step()
        restart = s._base_tree is None
        s._acceptances.append(bool(accept))
        s.append_chain(s.x, U=s._U)
        dbl = log['doublings']
        depth = sum(1 for d in dbl if not (d[2] or d[3]))
        us = uniform[n_u:]
        ps = draw_probabilities(cfg, dbl, log['merge_p'], restart, float(prob))
        assert len(us) == len(ps), (len(us), len(ps))
        for name, v in (('accept', bool(accept)), ('prob', float(prob)), ('U', float(s._U)), ('depth', depth),
                        ('H', np.nan if restart else float(s._base_tree.q_prop_H)), ('H_start', log['H_start']),
                        ('fn_evals', s.fn_evals - evals), ('restart', restart), ('dirs', [d[0] for d in dbl]), ('u', us),
                        ('nstates', 0 if restart or s._base_tree.states is None else len(s._base_tree.states))):
            rec[name].append(v)
        for name in nc.PER_LEAF:
            rec[name].append(list(log[name]))
        for k in nc.KEYS:
            xs[k].append(mg.npy(s.x[k]).copy())
        # what makes the record decisive
        last = dbl[-1]
        facts['turned_early'] |= last[3] and not last[2] and depth < cfg['max_tree_depth']
        facts['full_depth'] |= depth == cfg['max_tree_depth']
        facts['dirs'] |= {d[0] for d in dbl}
        facts['merges'] |= {u < p for u, p in zip(us, ps) if p not in (0.5,)} if not restart else set()
        facts['accepts'] |= set() if restart else {bool(accept)}
        facts['restart'] |= restart
        facts['late_div'] |= last[2] and depth >= 2 and not restart
        dH = np.array(log['leaf_H']) - log['H_start']
        ang = np.abs(np.array(log['leaf_minus'] + log['leaf_plus']))
        scale = np.array(log['angle_scale'][0::2] + log['angle_scale'][1::2])
        ok = (np.all(np.abs(np.array(us) - np.array(ps)) > nc.MARGIN) and np.all(np.abs(dH - cfg['dHmax']) > nc.MARGIN)
              and np.all(ang > nc.ANGLE_MARGIN * scale))
        facts['ok'] &= bool(ok)
        if verbose:
            print('  move %d: depth %d dirs %s leaves %d accept %s prob %.4f restart %s last (div %s, turn %s) max dH %.3f decisive %s'
                  % (i, depth, [int(d[0]) for d in dbl], len(log['leaf_K']), bool(accept), float(prob), restart, last[2], last[3],
                     dH.max(), ok))
    out = {}
    pre = 'chain_%s_' % tag
    for name in nc.PER_MOVE + ('nstates',):
        out[pre + name] = np.array(rec[name], dtype=float)
    for name in nc.PER_LEAF + ('u',):
        out[pre + name] = nc.padded(rec[name])
    out[pre + 'dirs'] = nc.padded(rec['dirs'], 0.0)
    for k in nc.KEYS:
        out[pre + 'x_' + k] = np.stack(xs[k])
    return out, facts


def check(tag, facts):
    assert facts['ok'], 'chain %s: a draw, an energy change or an angle is too close to its threshold' % tag
    if tag == 'a':
        assert facts['turned_early'] and facts['full_depth'], facts
        assert facts['dirs'] == {1.0, -1.0} and facts['merges'] == {True, False} and facts['accepts'] == {True, False}, facts
    if tag == 'b':
        assert facts['dirs'] == {1.0} and facts['merges'] == {True, False}, facts
    if tag == 'c':
        assert facts['restart'] and facts['late_div'], facts


def gen():
    sm, ParamDict = mgh.load_sampler()
    a, x0, cov, hess, _ = hc.chain_inputs(hc.golden())
    rng = np.random.default_rng(nc.DRAW_SEED)
    draws = {k: rng.normal(size=(nc.STEPS,) + hc.SHAPES[k]) for k in nc.KEYS}
    out = {'draws_' + k: draws[k] for k in nc.KEYS}
    uniform, rand = [], np.random.rand

    def recording_rand():
        uniform.append(rand())
        return uniform[-1]

    np.random.rand = recording_rand
    try:
        for tag in nc.CHAINS:
            print('chain %s: %s' % (tag, nc.CHAINS[tag]))
            arrs, facts = run_chain(sm, ParamDict, tag, a, cov, hess, x0, draws, uniform)
            check(tag, facts)
            out.update(arrs)
    finally:
        np.random.rand = rand
    mg.save('nuts', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen()
