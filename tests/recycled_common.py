"""
Shared by tests/test_recycled_host.py, tests/test_recycled_gpu.py and tests/golden/make_golden_recycled.py: the case tables, the
loader of tests/golden/recycled.npz, a numpy restatement of rime_hmc_recycle (hmc_common.oracle_step composed as the header
states it: half kick with the energy, snapshot, half kick and drift) with the bounds the GPU test asserts, a restatement of a
whole recycled move (momentum with its masks, the trajectory, the divergence restart, the Metropolis tests, the dynamic step size)
in float64 on the flat vector, and the tolerances.

Bounds of the recycle stage, from hmc_common (u the unit roundoff of T, uo of the long double restatement):
 * p_out = p1: one stage of the kick, B_1 = p_bound(p, g, eps, half).  q_out is a copy: exact.
 * energy: energy_bound(p1', B_1, c).
 * p = p2: a second kick on the computed p1, whose error it carries: B_2 = B_1 + p_bound(|p1'| + B_1, g, eps, half).
 * q: q_bound(q, p2', B_2, eps, c, drift).
Nothing here is fitted to what the kernel returns.

Tolerances of the chains:
 * float64: FACTOR x RESTATEMENT (floor FLOOR), as hmc_common.chain_discrepancy is used; RESTATEMENT is the largest relative
   discrepancy of the restated moves below against the reference's recorded chains (a) - (e), measured by the generator.
 * float32: decisions only.  They are the recorded ones if no Hamiltonian difference H_start - H_i moves by more than
   dH_bound(float32).  Its terms, relative to the largest recorded |H|: the potential is a sum per key of at most NTERMS positive
   terms of 4 roundings each, in any order (NTERMS + 4) u; the kinetic energy (E + 2) u with E = 16, its float64 part below u; the
   state reaches a Hamiltonian through at most Nstep + 1 stages of 2 (momentum) + 4 (position) roundings, each entering H
   through the gradient with sum |dH/dx x| <= 4 H for this potential (quadratic and quartic terms): 24 (Nstep + 1) u.  Both
   Hamiltonians of a difference carry it: the factor 2.  The host test checks every recorded margin against it.
"""
import math
import os

import numpy as np
import torch

import hmc_common as hc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'recycled.npz')

# measured 2026-10-21 (x86-64 CPU, numpy float64) by tests/golden/make_golden_recycled.py against the reference's chains; set by
# chain a; the decisions were equal
RESTATEMENT = 9.7e-14
TOL_CHAIN = max(hc.FACTOR * RESTATEMENT, hc.FLOOR)

KEYS = ('u', 'v', 'w')                                      # hmc_common.SHAPES; w is the complex key
TAGS = ('a', 'b', 'c', 'd', 'e')
NSTEP, MOVES = 5, 6
EPS = {'u': 0.30, 'v': 0.24, 'w': 0.27}
EPS_W_COMPLEX = 0.27 + 0.18j                                # chain b: the step of the complex key
DYN = dict(gamma=0.5, min_prob=0.6, alpha=2.0, index_key='v', index=(0, 64))     # chain c: powers of two, exact in any precision
# per chain: the seed of the host generator and dHmax
CHAINS = {'a': dict(seed=1, dHmax=1000.0), 'b': dict(seed=2, dHmax=1000.0), 'c': dict(seed=1, dHmax=1000.0),
          'd': dict(seed=1, dHmax=1000.0), 'e': dict(seed=2, dHmax=0.5)}

# the kernel's shapes: nothing, a lone element, a ragged wave, one element either side of a chunk of either precision, three
# work-groups and a tail
KERNEL_NS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 5)
ORACLE_N = 4097
NTERMS = max(int(np.prod(s)) * (2 if k == 'w' else 1) for k, s in hc.SHAPES.items())

_CACHE = {}


def golden():
    """recycled.npz as a dict of numpy arrays, loaded once and never modified by a test"""
    if GOLDEN not in _CACHE:
        with np.load(GOLDEN) as f:
            _CACHE[GOLDEN] = {k: f[k] for k in f.files}
    return _CACHE[GOLDEN]


def second_trip_N(maxblocks, span):
    """one N beyond the largest grid by a chunk and a tail: the grid-stride loop takes a second trip in some work-groups"""
    return maxblocks * span + span + 5


def dH_bound(dtype, Hmax, Nstep=NSTEP):
    """how far a difference of two Hamiltonians of a chain may move in the working precision (the derivation is above)"""
    E = 16 if dtype in (torch.float32, np.float32) else 8
    return 2 * ((NTERMS + 4) + (E + 2) + 1 + 24 * (Nstep + 1)) * hc.unit(dtype) * Hmax


# ----------------------------------------------------------------------------------------------- the stage restated with bounds
def oracle_recycle(q, p, g, eps, c, half, drift, dtype):
    """
    rime_hmc_recycle in long double on the operands as the kernel sees them: returns (q', p', q_out', p_out', E') and the bounds
    (B_q, B_p, B_pout, B_E) of the kernel's results around them.
    """
    _, p1, E = hc.oracle_step(q, p, g, eps, c, half, 0.0, dtype)
    B1 = hc.p_bound(p, g, eps, half, dtype)
    BE = hc.energy_bound(p1, B1, c, dtype, float(E))
    q_out = hc._ld(q)
    if drift == 0:
        return q_out, p1, q_out, p1, E, (np.zeros_like(p1), B1, B1, BE)
    q2, p2, _ = hc.oracle_step(q, p1, g, eps, c, half, drift, dtype)
    B2 = B1 + hc.p_bound(np.abs(p1) + B1, g, eps, half, dtype)
    Bq = hc.q_bound(q, p2, B2, eps, c, drift, dtype)
    return q2, p2, q_out, p1, E, (Bq, B2, B1, BE)


# ----------------------------------------------------------------------------------------------- the flat vector, in numpy
class Flat:
    """sampler._Layout's rule restated: keys in order, a complex key on an even element as interleaved (re, im)"""

    def __init__(self, x):
        self.keys, self.slices, self.shapes, self.cplx = list(x), {}, {}, {}
        n = 0
        for k in self.keys:
            cp = np.iscomplexobj(x[k])
            n += (n & 1) if cp else 0
            m = x[k].size * (2 if cp else 1)
            self.slices[k], self.shapes[k], self.cplx[k] = slice(n, n + m), x[k].shape, cp
            n += m
        self.N = n

    def pack(self, d, fill=0.0):
        """a dict of arrays as the flat float64 vector; a real value of a complex key is repeated per component"""
        out = np.full(self.N, fill)
        for k in self.keys:
            v = np.broadcast_to(np.asarray(d[k]), self.shapes[k])
            if self.cplx[k]:
                v = np.stack([v.real, v.imag], -1) if np.iscomplexobj(v) else np.stack([v, v], -1)
            out[self.slices[k]] = v.reshape(-1)
        return out

    def unpack(self, flat):
        out = {}
        for k in self.keys:
            v = flat[self.slices[k]]
            out[k] = (v[0::2] + 1j * v[1::2]).reshape(self.shapes[k]) if self.cplx[k] else v.reshape(self.shapes[k]).copy()
        return out


def mul_eps(x, e):
    """recycled.multiply_eps in numpy"""
    if e is None:
        return x
    return x.real * e.real + 1j * (x.imag * e.imag) if np.iscomplexobj(e) else x * e


class OracleDyn:
    """recycled.DynamicStepSize restated: floats per key, an index (slice) per key or None"""

    def __init__(self, params, gamma, min_prob, alpha, index=None):
        self.params, self.gamma, self.min_prob, self.alpha, self.index = params, gamma, min_prob, alpha, index
        self.eps_mul = {k: 1.0 for k in params}

    def effective(self):
        out = {}
        for k, v in self.params.items():
            out[k] = np.array(v, dtype=np.result_type(v, np.float64))
            out[k][self.index[k] if self.index is not None else Ellipsis] *= self.eps_mul[k]
        return out

    def update(self, prob):
        for k, v in self.eps_mul.items():
            self.eps_mul[k] = v * self.gamma if prob < self.min_prob else min(v * self.alpha, 1.0)


def _f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


class OracleRecycled:
    """one chain of recycled.RecycledHMC in float64 numpy on the flat vector, every stage through hmc_common.oracle_step"""

    def __init__(self, a, x0, eps, cov, hess, Nstep, dHmax, draws, pmask=None, dyn=None):
        self.lay = Flat(x0)
        self.grad, self.x, self.eps, self.cov, self.hess = hc.chain_potential(a), dict(x0), eps, cov, hess
        self.c = self.lay.pack(cov, fill=1.0)
        self.Nstep, self.dHmax, self.draws, self.ndrawn, self.pmask, self.dyn = Nstep, dHmax, draws, 0, pmask, dyn
        self.logdetM = sum(2 * np.log(hess[k]).sum() for k in hess)
        self.chain, self.Uchain, self.acceptances = [], [], []
        self.U, self.g = self.grad(self.x)
        # the masks on the flat vector (a key without one: ones); the reference's K() multiplies the momentum by it in place
        self.m = None if pmask is None else self.lay.pack({k: (1.0 if pmask[k] is None else pmask[k]) for k in self.x}, fill=1.0)

    def momentum(self):
        p = {}
        for k in self.x:
            mask = None if self.pmask is None else self.pmask[k]
            p[k] = mul_eps(self.hess[k] * mul_eps(self.draws[k][self.ndrawn], mask), mask)
        self.ndrawn += 1
        return self.lay.pack(p)

    def finish(self, prob):
        if self.dyn is not None:
            self.dyn.update(prob)

    def step(self):
        lay, c, f = self.lay, self.c, np.float64
        eps = lay.pack(self.dyn.effective() if self.dyn is not None else self.eps, fill=1.0)
        q, p = lay.pack(self.x), self.momentum()
        if self.m is not None:
            p = p * self.m
        K_start = float(hc.oracle_step(q, p, None, None, c, 0.0, 0.0, f)[2]) + self.logdetM
        U_start, g_start = self.U, self.g
        H_start = K_start + float(U_start)
        q, p = _f64(*hc.oracle_step(q, p, lay.pack(g_start), eps, c, 0.5, 1.0, f)[:2])
        rec = dict(H_start=H_start, H=[], u=[], accept=[], div=False, prob=0.0)
        rows, Us, gs = [], [], []
        for i in range(self.Nstep):
            self.U, self.g = self.grad(lay.unpack(q))
            drift = 0.0 if i == self.Nstep - 1 else 1.0
            if self.m is None:
                q, p, qo, _, E, _ = oracle_recycle(q, p, lay.pack(self.g), eps, c, 0.5, drift, f)
            else:                                    # the unfused sequence with the mask after the closing kick
                p = _f64(hc.oracle_step(q, p, lay.pack(self.g), eps, c, 0.5, 0.0, f)[1])[0] * self.m
                qo, E = q, hc.oracle_step(q, p, None, None, c, 0.0, 0.0, f)[2]
                if drift:
                    q, p = hc.oracle_step(q, p, lay.pack(self.g), eps, c, 0.5, drift, f)[:2]
            q, p, qo = _f64(q, p, qo)
            rec['H'].append(float(self.U) + float(E) + self.logdetM)
            if rec['H'][-1] - H_start > self.dHmax:
                if len(self.Uchain) > 0:
                    j = np.random.randint(0, len(self.Uchain))
                    self.U, self.x = self.Uchain[j], dict(self.chain[j])
                rec['div'] = True
                self.finish(0.0)
                return self.close(rec)
            rows.append(qo), Us.append(self.U), gs.append(self.g)
        self.U, self.g = U_start, g_start
        for i in range(self.Nstep):
            prob = min(1.0, math.exp(H_start - rec['H'][i]))
            rec['u'].append(np.random.rand())
            accept = bool(rec['u'][-1] < prob)
            if accept:
                self.x, self.U, self.g = lay.unpack(rows[i]), Us[i], gs[i]
                self.chain.append(dict(self.x))
                self.Uchain.append(self.U)
            rec['accept'].append(accept)
            self.acceptances.append(accept)
        rec['prob'] = prob
        self.finish(prob)
        return self.close(rec)

    def close(self, rec):
        rec.update(U=float(self.U), x=dict(self.x), nchain=len(self.Uchain),
                   eps_mul=None if self.dyn is None else dict(self.dyn.eps_mul))
        return rec


# ----------------------------------------------------------------------------------------------- the recorded chains
def chain_setup(g, tag):
    """
    What chain `tag` is run with, as numpy: (a, x0, cov, hess, draws, eps, pmask, dyn arguments or None, dHmax).  eps: a dict per
    key of a float, a complex number (chain b, key w) or, for chain c, the nominal step as an array of the parameter's shape.
    """
    get = lambda name: {k: g['in_%s_%s' % (name, k)] for k in KEYS}
    eps, pmask, dyn = dict(EPS), None, None
    if tag == 'b':
        eps['w'] = EPS_W_COMPLEX
    if tag == 'c':
        eps = {k: np.full(hc.SHAPES[k], EPS[k]) for k in KEYS}
        dyn = dict(gamma=DYN['gamma'], min_prob=DYN['min_prob'], alpha=DYN['alpha'],
                   index={k: (slice(*DYN['index']) if k == DYN['index_key'] else slice(None)) for k in KEYS})
    if tag == 'd':
        pmask = get('mask')                          # real on u, ones on v (recycled is given None there), complex on w
    return get('a'), get('x0'), get('cov'), get('hess'), get('draws'), eps, pmask, dyn, CHAINS[tag]['dHmax']


def run_oracle_chain(g, tag):
    a, x0, cov, hess, draws, eps, pmask, dyn, dHmax = chain_setup(g, tag)
    np.random.seed(CHAINS[tag]['seed'])
    h = OracleRecycled(a, x0, eps, cov, hess, NSTEP, dHmax, draws, pmask=pmask,
                       dyn=None if dyn is None else OracleDyn(eps, dyn['gamma'], dyn['min_prob'], dyn['alpha'], dyn['index']))
    return [h.step() for _ in range(MOVES)]


def oracle_hmc_move(g, Nstep, masked=True):
    """
    One move of recycled.HMC from x0 with the first recorded draws, the steps of chain a and the masks of chain d applied in
    draw_momentum only, in float64 numpy through hmc_common.oracle_step: (K_start, H_start, H_end, prob, the final position).
    """
    a, x0, cov, hess, draws, eps, _, _, _ = chain_setup(g, 'a')
    h = OracleRecycled(a, x0, eps, cov, hess, Nstep, np.inf, draws, pmask=chain_setup(g, 'd')[6] if masked else None)
    lay, c, f = h.lay, h.c, np.float64
    e = lay.pack(eps, fill=1.0)
    q, p = lay.pack(h.x), h.momentum()
    K_start = float(hc.oracle_step(q, p, None, None, c, 0.0, 0.0, f)[2]) + h.logdetM
    U, gr = h.grad(h.x)
    for i in range(Nstep):
        q, p = _f64(*hc.oracle_step(q, p, lay.pack(gr), e, c, 0.5 if i == 0 else 1.0, 1.0, f)[:2])
        U_end, gr = h.grad(lay.unpack(q))
    _, p, E = hc.oracle_step(q, p, lay.pack(gr), e, c, 0.5, 0.0, f)
    H_start, H_end = K_start + float(U), float(E) + h.logdetM + float(U_end)
    return K_start, H_start, H_end, min(1.0, math.exp(H_start - H_end)), lay.unpack(q)


def padded(rows, n=NSTEP):
    """a ragged list of lists as a (len, n) float array, NaN where a move ended early"""
    out = np.full((len(rows), n), np.nan)
    for i, r in enumerate(rows):
        out[i, :len(r)] = np.asarray(r, dtype=float)
    return out


def decisions(recs):
    """(accept, div, nchain) of per-move records as arrays; accept NaN-padded"""
    return (padded([r['accept'] for r in recs]), np.array([float(r['div']) for r in recs]),
            np.array([float(r['nchain']) for r in recs]))


def same_decisions(recs, g, tag):
    acc, div, nchain = decisions(recs)
    return (np.array_equal(acc, g[tag + '_accept'], equal_nan=True) and np.array_equal(div, g[tag + '_div'])
            and np.array_equal(nchain, g[tag + '_nchain']))


def chain_discrepancy(recs, g, tag):
    """
    Largest relative discrepancy of per-move records (dicts with H_start, H, prob, U, x, accept, div, nchain) against the recorded
    chain `tag`, each quantity relative to its largest recorded magnitude; the decisions must be equal.
    """
    assert same_decisions(recs, g, tag), (decisions(recs), g[tag + '_accept'], g[tag + '_div'], g[tag + '_nchain'])
    worst = 0.0
    for name in ('H_start', 'prob', 'U'):
        ref = g['%s_%s' % (tag, name)]
        worst = max(worst, float(np.abs(np.array([float(r[name]) for r in recs]) - ref).max() / np.abs(ref).max()))
    ref, got = g[tag + '_H'], padded([r['H'] for r in recs])
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    worst = max(worst, float(np.nanmax(np.abs(got - ref)) / np.nanmax(np.abs(ref))))
    for k in KEYS:
        ref = g['%s_x_%s' % (tag, k)]
        worst = max(worst, float(np.abs(np.stack([np.asarray(r['x'][k]) for r in recs]) - ref).max() / np.abs(ref).max()))
    return worst


def eps_mul_of(recs):
    """(moves, keys) array of the multipliers after every move of chain c"""
    return np.array([[float(r['eps_mul'][k]) for k in KEYS] for r in recs])
