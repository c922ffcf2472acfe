"""
Shared by tests/test_nuts_host.py, tests/test_nuts_gpu.py and tests/golden/make_golden_nuts.py: the fixture loader of
tests/golden/nuts.npz, the table of recorded chains the generator and the tests walk together, a long-double restatement of the
two tree-leaf kernels of csrc/nuts.hip,

    open:    p1 = p0 - (T(h/2) * eps) * g0;     q1 = q0 + (T(h) * eps) * (c * (c * p1))
    close:   p1 <- p1 - (T(h/2) * eps) * g1;    out = (1/2 sum (c * p1)^2,  sum (q1 - q_far) * p_far,  sum (q1 - q_far) * p1)

the rounding bounds of the two projections, and OracleNUTS: the algorithm of the reference's sampler.NUTS in plain float64 numpy,
without the package.  The potential, the shapes, the inputs (a, x0, cov, hess) and the restatement of one kernel stage come
from tests/hmc_common.py: open is its oracle_step with (kick, drift) = (h/2, h), the momentum of close and out[0] its
oracle_step with (h/2, 0) and the energy, and p_bound, q_bound and energy_bound hold as they stand.

Bounds of the projections, with u, u64, uo and gamma_n as in hmc_common, E = 64 / sizeof(T) the elements of a lane, d = q1 -
q_far, p' the restatement's updated momentum and B_p its bound.  The kernel rounds d once in T and runs a chain of E fused
multiply-adds in T per lane, so a term d_i x_i carries at most E + 1 roundings; the lanes' values are then added in float64,
each passing through at most n64 additions (hmc_common.energy_bound: 6 + chunks per work-group + 3 + ceil(work-groups / 64)
+ 6).  q1, q_far and p_far are operands the kernel and the restatement share; the momentum of out[2] is the kernel's own, within
B_p of p'.  The restatement rounds d, the product and at most no = 128 + ceil(log2 N) + 3 partial sums in long double:
    G = gamma_{E+1}(u) + gamma_n64(u64) (1 + gamma_{E+1}(u))
    |out1^ - out1'| <= G sum |d| |p_far|                               + gamma_no(uo) sum |d| |p_far|            dots_bound()[0]
    |out2^ - out2'| <= G sum |d| (|p'| + B_p)  +  sum |d| B_p          + gamma_no(uo) sum |d| |p'|               dots_bound()[1]
A bound that is zero asks for the exact value.  Nothing here is fitted to what the kernels return.

NUTS_RESTATEMENT: the largest relative discrepancy max|x - x_ref| / max|x_ref| of OracleNUTS against the three recorded chains
(prob, U, the proposal's H, x per move; K and the two angles per leaf), with every decision equal: accept, tree depth, fn_evals,
the directions, the number of leaves and of uniform draws.  Measured on the CPU against the REFERENCE's record, never against
the GPU code; the tests assert at hmc_common.FACTOR times it plus hmc_common.FLOOR: the restatement and the reference differ by
rounding order only, while an algorithmic slip (a wrong edge, weight or sign) changes a decision or shows at the 1e-2 level.
"""
import math
import os

import numpy as np

import hmc_common as hc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nuts.npz')
_CACHE = {}

FACTOR, FLOOR, MARGIN = hc.FACTOR, hc.FLOOR, hc.MARGIN
# measured 2026-10-20 (x86-64 CPU, numpy float64) against tests/golden/nuts.npz; set by prob of chain 'c' (chain 'a': 5.5e-14, also
# prob, the exponential of a difference of Hamiltonians near 400; chain 'b': 2.3e-16; everything but prob: below 3.4e-16)
NUTS_RESTATEMENT = 9.69e-14
ANGLE_MARGIN = 1e-3                                        # every recorded angle: |angle| > ANGLE_MARGIN sum |q1 - q_far| |p|

KEYS = hc.CHAIN['keys']
STEPS = 6
DRAW_SEED = 4021                                           # of the recorded momentum draws
# tag: what the generator passes to the reference's NUTS beside the potential, the start and the Cholesky factors
CHAINS = {
    'a': dict(seed=11, eps=0.4, max_tree_depth=3, dHmax=1000.0, biased=True, sample_direction=True, track_states=False),
    'b': dict(seed=12, eps=0.4, max_tree_depth=3, dHmax=1000.0, biased=False, sample_direction=False, track_states=True),
    'c': dict(seed=15, eps=0.5, max_tree_depth=4, dHmax=1.5, biased=True, sample_direction=True, track_states=False),
}
PER_MOVE = ('accept', 'prob', 'U', 'H', 'H_start', 'depth', 'fn_evals', 'restart')
PER_LEAF = ('leaf_K', 'leaf_H', 'leaf_minus', 'leaf_plus')


def golden():
    """nuts.npz as a dict of numpy arrays, loaded once and never modified by a test"""
    if GOLDEN not in _CACHE:
        with np.load(GOLDEN) as f:
            _CACHE[GOLDEN] = {k: f[k] for k in f.files}
    return _CACHE[GOLDEN]


def chain_inputs(g):
    """(a, x0, cov, hess) of hmc.npz's chains and the momentum draws of nuts.npz, dicts of float64 numpy arrays by key"""
    a, x0, cov, hess, _ = hc.chain_inputs(hc.golden())
    return a, x0, cov, hess, {k: g['draws_' + k] for k in KEYS}


# --------------------------------------------------------------------------------------------- restatement of the kernels
def oracle_open(q0, p0, g0, eps, c, h, dtype):
    """(q1', p1') in long double"""
    q, p, _ = hc.oracle_step(q0, p0, g0, eps, c, h / 2, h, dtype)
    return q, p


def oracle_close(q1, p1, g1, eps, c, h, q_far, p_far, dtype):
    """(p1', (out0', out1', out2')) in long double; the projections are None without a far edge"""
    _, p, E = hc.oracle_step(None, p1, g1, eps, c, h / 2, 0.0, dtype)
    if q_far is None:
        return p, (E, None, None)
    d = hc._ld(q1) - hc._ld(q_far)
    return p, (E, (d * hc._ld(p_far)).sum(), (d * p).sum())


def dots_bound(q1, q_far, p_far, p1, Bp, dtype):
    """bounds of out[1] and out[2]; p1 the restatement's updated momentum, Bp its bound"""
    d = np.abs(hc._ld(q1) - hc._ld(q_far)) * (1 + hc.UO)
    N = d.size
    E = 16 if hc.unit(dtype) == 2.0 ** -24 else 8
    nchunks = -(-N // (256 * E))
    nblocks = min(nchunks, 1024)
    n64 = 6 + -(-nchunks // max(nblocks, 1)) + 3 + -(-nblocks // 64) + 6
    gT = hc.gamma_n(E + 1, hc.unit(dtype))
    G = gT + hc.gamma_n(n64, 2.0 ** -53) * (1 + gT)
    go = hc.gamma_n(128 + int(math.ceil(math.log2(max(N, 2)))) + 3, hc.UO)
    apf, ap = np.abs(hc._ld(p_far)), np.abs(p1)
    return (float((G + go) * (d * apf).sum()),
            float(G * (d * (ap + Bp)).sum() + (d * Bp).sum() + go * (d * ap).sum()))


def within(got, want, B):
    """|got - want| <= B; a zero bound asks for the exact value"""
    err = abs(np.longdouble(got) - np.longdouble(want))
    return bool(err == 0) if B == 0 else bool(err <= B)


# ------------------------------------------------------------------------------------------------- restatement of the move
def _logaddexp(x, y):
    lo, hi = (x, y) if x < y else (y, x)
    return math.log1p(math.exp(lo - hi)) + hi


def angles(q_far, p_far, q1, p1, direction):
    """(minus, plus) of the reference's hoffman_uturn between the far edge and a leaf, and the scale sum |q1 - q_far| |p| of each"""
    far = sum(float(((q1[k] - q_far[k]) * p_far[k]).sum()) for k in q1)
    near = sum(float(((q1[k] - q_far[k]) * p1[k]).sum()) for k in q1)
    sfar = sum(float((np.abs(q1[k] - q_far[k]) * np.abs(p_far[k])).sum()) for k in q1)
    snear = sum(float((np.abs(q1[k] - q_far[k]) * np.abs(p1[k])).sum()) for k in q1)
    return ((far, near), (sfar, snear)) if direction > 0 else ((-near, -far), (snear, sfar))


class OracleNUTS:
    """one chain in float64 numpy: the algorithm of the reference's sampler.NUTS restated without the package"""

    def __init__(self, a, x0, eps, cov, hess, draws, dHmax, max_tree_depth, biased, sample_direction, track_states, **_):
        self.grad, self.x, self.eps, self.cov, self.hess = hc.chain_potential(a), dict(x0), eps, cov, hess
        self.dHmax, self.max_tree_depth, self.biased = dHmax, max_tree_depth, biased
        self.sample_direction, self.track_states = sample_direction, track_states
        self.draws, self.ndrawn, self.fn_evals = draws, 0, 0
        self.logdetM = sum(2 * np.log(hess[k]).sum() for k in hess)
        self.chain, self.Uchain = [], []
        self.U = self.potential(self.x)[0]

    def potential(self, q):
        self.fn_evals += 1
        U, g = self.grad(q)
        return float(U), g

    def K(self, p):
        return float(sum(((self.cov[k] * p[k]) ** 2).sum() / 2 for k in p) + self.logdetM)

    def rand(self):
        self.rec['u'].append(np.random.rand())
        return self.rec['u'][-1]

    def append_chain(self):
        self.chain.append(dict(self.x))
        self.Uchain.append(self.U)

    def leaf(self, edge, direction, H_start, far):
        q, p, g = edge
        e = direction * self.eps
        p = {k: p[k] - (0.5 * e) * g[k] for k in p}
        q = {k: q[k] + e * (self.cov[k] * (self.cov[k] * p[k])) for k in q}
        U, g = self.potential(q)
        p = {k: p[k] - (0.5 * e) * g[k] for k in p}
        K = self.K(p)
        H = U + K
        (minus, plus), _ = angles(far[0], far[1], q, p, direction)
        for name, v in (('leaf_K', K), ('leaf_H', H), ('leaf_minus', minus), ('leaf_plus', plus)):
            self.rec[name].append(v)
        s = (q, p, g)
        return dict(left=s, right=s, prop=s, U=U, H=H, weight=_logaddexp(-H_start, -H), turning=False,
                    diverging=(H - H_start) > self.dHmax, states=[(q, p, U)] if self.track_states else None,
                    angles=(minus, plus))

    def merge(self, old, new, new_right):
        d = new['weight'] - (old['weight'] if self.biased else _logaddexp(old['weight'], new['weight']))
        keep = new if self.rand() < (1.0 if d >= 0 else math.exp(d)) else old
        left, right = (old, new) if new_right else (new, old)
        return dict(left=left['left'], right=right['right'], prop=keep['prop'], U=keep['U'], H=keep['H'],
                    weight=_logaddexp(old['weight'], new['weight']), turning=old['turning'] or new['turning'],
                    diverging=old['diverging'] or new['diverging'],
                    states=None if old['states'] is None else left['states'] + right['states'], angles=new['angles'])

    def build(self, edge, direction, depth, H_start, far):
        if depth == 0:
            return self.leaf(edge, direction, H_start, far)
        half = self.build(edge, direction, depth - 1, H_start, far)
        other = self.build(half['right'] if direction > 0 else half['left'], direction, depth - 1, H_start, far)
        merged = self.merge(half, other, direction > 0)
        minus, plus = merged['angles']                      # those of the outer leaf, against the base tree's far edge
        merged['turning'] = merged['turning'] or (minus < 0) or (plus < 0)
        return merged

    def step(self):
        evals = self.fn_evals
        self.rec = rec = dict(u=[], dirs=[], leaf_K=[], leaf_H=[], leaf_minus=[], leaf_plus=[])
        p = {k: self.hess[k] * self.draws[k][self.ndrawn] for k in self.x}
        self.ndrawn += 1
        K_start = self.K(p)
        U_start, g = self.potential(self.x)
        H_start = K_start + U_start
        s = (dict(self.x), p, g)
        base = dict(left=s, right=s, prop=s, U=U_start, H=H_start, weight=-H_start, turning=False, diverging=False,
                    states=[(s[0], p, U_start)] if self.track_states else None, angles=None)
        depth, new, direction = 0, None, 1.0
        while depth < self.max_tree_depth:
            direction = (1.0 if self.rand() > 0.5 else -1.0) if self.sample_direction else 1.0
            rec['dirs'].append(direction)
            new = self.build(base['right'] if direction > 0 else base['left'], direction, depth, H_start,
                             base['left'] if direction > 0 else base['right'])
            if new['diverging'] or new['turning']:
                break
            base = self.merge(base, new, direction > 0)
            depth += 1
        rec.update(depth=depth, H_start=H_start, H=base['H'], restart=False, states=base['states'])
        if new['diverging'] and len(self.Uchain) > 0 and depth < 2:
            i = np.random.randint(0, len(self.Uchain))
            self.U, self.x = self.Uchain[i], dict(self.chain[i])
            rec.update(accept=False, prob=0.0, H=np.nan, restart=True)
        else:
            d = H_start - base['H']
            prob = min(1.0, math.exp(min(d, 700.0)))
            accept = bool(self.rand() < prob)
            if accept:
                self.x, self.U = dict(base['prop'][0]), base['U']
            else:
                self.U = U_start
            rec.update(accept=accept, prob=prob)
        rec.update(U=self.U, x=dict(self.x), fn_evals=self.fn_evals - evals)
        return rec


def run_oracle_chain(g, tag):
    a, x0, cov, hess, draws = chain_inputs(g)
    cfg = CHAINS[tag]
    np.random.seed(cfg['seed'])
    s = OracleNUTS(a, x0, cfg['eps'], cov, hess, draws, **{k: v for k, v in cfg.items() if k not in ('seed', 'eps')})
    recs = []
    for _ in range(STEPS):
        recs.append(s.step())
        s.append_chain()
    return recs


def padded(rows, fill=np.nan):
    """a list of lists of numbers as one float64 array, short rows filled"""
    out = np.full((len(rows), max(1, max(len(r) for r in rows))), fill)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def chain_discrepancy(recs, g, tag, values=('prob', 'U', 'H', 'leaf_K', 'leaf_H', 'leaf_minus', 'leaf_plus', 'x')):
    """
    Largest relative discrepancy of the per-move records `recs` (dicts as OracleNUTS.step returns them; `u` may be missing)
    against the recorded chain `tag`, each quantity relative to its largest recorded magnitude; the decisions must be equal.
    """
    pre = 'chain_%s_' % tag
    for name in ('accept', 'restart', 'depth', 'fn_evals'):
        assert [float(r[name]) for r in recs] == g[pre + name].tolist(), (name, [r[name] for r in recs], g[pre + name])
    assert np.array_equal(padded([r['dirs'] for r in recs], 0.0), g[pre + 'dirs'])
    if 'u' in recs[0]:
        assert np.array_equal(padded([r['u'] for r in recs]), g[pre + 'u'], equal_nan=True)
    worst = 0.0
    for name in values:
        if name == 'x':
            pairs = [(np.stack([np.asarray(r['x'][k]) for r in recs]), g[pre + 'x_' + k]) for k in KEYS]
        elif name in PER_LEAF:
            pairs = [(padded([r[name] for r in recs]), g[pre + name])]
        else:
            pairs = [(np.array([float(r[name]) for r in recs]), g[pre + name])]
        for got, ref in pairs:
            assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), name
            ok = ~np.isnan(ref)
            worst = max(worst, float(np.abs(got[ok] - ref[ok]).max() / np.abs(ref[ok]).max()))
    return worst
