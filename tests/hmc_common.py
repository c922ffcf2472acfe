"""
Shared by tests/test_hmc_host.py, tests/test_hmc_gpu.py and tests/golden/make_golden_hmc.py: the fixture loader of
tests/golden/hmc.npz, the case tables the generator and the tests walk together, the separable potential of the fixtures, a
plain numpy restatement of rime_hmc_step,

    kick  != 0:   p <- p - (T(kick) * eps) * g
    drift != 0:   q <- q + (T(drift) * eps) * (c * (c * p))      with the updated p
    energy:       E = 1/2 sum (c * p)^2                          with the updated p

of leapfrog and of a whole HMC move (momentum, trajectory, Metropolis decision, divergence restart) on it, and the accuracy
bounds the GPU tests assert.  The restatement runs on the ROUNDED operands (q, p, g, eps, c as the kernel sees them, kick and
drift rounded to T) in numpy's long double where the kernel's element chains are compared (oracle_step), so that its own
rounding, uo = half the long double epsilon of the machine the test runs on, is small beside float64's; it is counted anyway.

Bounds, with u = 2^-24 (float32) or 2^-53 (float64) for the working precision T, u64 = 2^-53, gamma_n(u) = n u / (1 - n u)
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), p', q' the restatement's results:

 * p.  One rounding for T(kick) * eps and one for the fused multiply-add (the negation is exact):
       |p^ - p'| <= B_p = (gamma_2(u) + gamma_3(uo)) (|p| + |kick eps g|)                                          p_bound()
   (the restatement: product, product, subtraction).
 * q.  Four roundings -- T(drift) * eps, c * p, c * (c p), the fused multiply-add -- plus the propagated error of p scaled by
   s = |drift eps c^2|:  q^ = (q + drift eps c^2 p^ theta_3)(1 + delta), so
       |q^ - q'| <= B_q = gamma_4(u) (|q| + s (|p'| + B_p)) + s B_p + gamma_5(uo) (|q| + s |p'|)                   q_bound()
 * energy.  The dots bound of lbfgs_common with the chain lengthened by the c * p products: a lane adds its E = 64 / sizeof(T)
   squares in one chain of E fused multiply-adds in T, each square of a product that was rounded once: E + 2 factors.  Then
   float64 additions, each value passing through at most
       n64 = 6 (butterfly of a wave) + C (chunks of a work-group, C = ceil(nchunks / nblocks)) + 3 (waves of a work-group)
             + ceil(nblocks / 64) (partials a lane of the second stage adds) + 6 (its butterfly)
   of them (the halving is exact), nchunks = ceil(N / (256 E)), nblocks = min(nchunks, 1024).  With the propagated error of p
   and the restatement's own sum (numpy adds blocks of at most 128 terms naively and the blocks pairwise: at most
   no = 128 + ceil(log2 N) + 3 roundings on the way of a term, the 3 for c * p and the square):
       |E^ - E'| <= (gamma_{E+2}(u) + gamma_n64(u64) (1 + gamma_{E+2}(u))) 1/2 sum c^2 (|p'| + B_p)^2
                    + 1/2 sum c^2 (2 |p'| B_p + B_p^2) + gamma_no(uo) E'                                            energy_bound()
An element whose bound is zero must be exact.  Nothing here is fitted to what the kernel returns.

Recorded constants (measured against the REFERENCE's recorded outputs, never against the GPU code; the tests assert at
FACTOR = 100 times them: the restatement and the reference differ by rounding order only, while any algorithmic slip shows at
eps^2 ~ 1e-2):
 * LEAP_RESTATEMENT: the largest relative discrepancy max|x - x_ref| / max|x_ref| of oracle_leapfrog (float64) against the
   recorded leapfrog outputs, over q and p of every case of LEAP_CASES.
 * CHAIN_RESTATEMENT: the same of run_oracle_chain (OracleHMC) against the recorded chains 'b' and 'c' (prob, U, x, p,
   K_start, H_end per move) and of OracleHMC.dual_averaging against record 'd'; the decisions were equal.
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hmc.npz')
_CACHE = {}

FACTOR = 100.0
FLOOR = 1e-13                # rounding-order slack relative to the largest recorded magnitude (GPU runs against the records)
# measured 2026-10-18 (x86-64 CPU, numpy float64) against tests/golden/hmc.npz; set by the case d_elem_cplx (t_scalar: 0,
# d_scalar 4.1e-17, d_key_cov with its states 7.7e-17, t_elem_cov 1.1e-16)
LEAP_RESTATEMENT = 1.86e-16
# measured the same day; set by chain 'b' (chain 'c': 5.5e-16, dual averaging: 0); the decisions were equal
CHAIN_RESTATEMENT = 7.44e-15

# ------------------------------------------------------------------------------------------------------------ the fixtures
SHAPES = {'u': (3, 70), 'v': (129,), 'w': (17,)}           # w is the complex key
QUARTIC = 0.1                                              # U = sum a x^2 / 2 + QUARTIC x^4 / 4  (complex keys: a |x|^2 / 2)
LEAP_N = 5
# name: (container, keys, eps kind, with cov_L)
LEAP_CASES = {
    't_scalar': ('tensor', ('v',), 'scalar', False),
    't_elem_cov': ('tensor', ('u',), 'elem', True),
    'd_scalar': ('pdict', ('u', 'v'), 'scalar', False),
    'd_key_cov': ('pdict', ('u', 'v'), 'key', True),
    'd_elem_cplx': ('pdict', ('u', 'v', 'w'), 'elem', True),
}
LEAP_STATES = 'd_key_cov'                                   # the case whose `states` are recorded
EPS_SCALAR = 0.05
CHAIN = dict(keys=('u', 'v'), Nstep=7, steps=6, seed=1234, eps={'u': 0.55, 'v': 0.4}, dHmax_b=1000.0, dHmax_c=0.7,
             Nadapt=5, dual_scale=0.1)       # dual averaging starts from dual_scale * eps (its first iterate is ~10 x the start)
MARGIN = 1e-3


def golden():
    """hmc.npz as a dict of numpy arrays, loaded once and never modified by a test"""
    if GOLDEN not in _CACHE:
        with np.load(GOLDEN) as f:
            _CACHE[GOLDEN] = {k: f[k] for k in f.files}
    return _CACHE[GOLDEN]


def grad_U(a, x, quartic=QUARTIC):
    """(U, dU/dx) of one key of the separable potential, any array library (numpy arrays or torch tensors)"""
    if 'complex' in str(x.dtype):
        return (a * (x.real ** 2 + x.imag ** 2)).sum() / 2, a * x
    return (a * x * x / 2 + quartic * x ** 4 / 4).sum(), a * x + quartic * x ** 3


# ------------------------------------------------------------------------------------------------- restatement of the kernel
def unit(dtype):
    return 2.0 ** -24 if dtype in (torch.float32, np.float32) else 2.0 ** -53


def gamma_n(n, u):
    return n * u / (1 - n * u)


UO = float(np.finfo(np.longdouble).eps) / 2


def _ld(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t).astype(np.longdouble)


def round_to(x, dtype):
    """the scalar x as the kernel's T(x)"""
    return float(np.float32(x)) if dtype in (torch.float32, np.float32) else float(x)


def oracle_step(q, p, g, eps, c, kick, drift, dtype):
    """(q', p', E') in long double from the operands as the kernel sees them; kick, drift as given to the entry point"""
    q, p, g, eps, c = _ld(q), _ld(p), _ld(g), _ld(eps), _ld(c)
    one = np.longdouble(1)
    k, d = np.longdouble(round_to(kick, dtype)), np.longdouble(round_to(drift, dtype))
    eps = one if eps is None else eps
    if kick != 0:
        p = p - (k * eps) * g
    z = p if c is None else c * p
    if drift != 0:
        q = q + (d * eps) * (z if c is None else c * z)
    return q, p, (z * z).sum() / 2


def p_bound(p, g, eps, kick, dtype):
    p, g, eps = _ld(p), _ld(g), _ld(eps)
    if kick == 0:
        return np.zeros_like(p)
    kg = abs(round_to(kick, dtype)) * np.abs(g) * (1 if eps is None else np.abs(eps))
    return (gamma_n(2, unit(dtype)) + gamma_n(3, UO)) * (np.abs(p) + kg)


def q_bound(q, p1, Bp, eps, c, drift, dtype):
    """p1: the restatement's updated momentum, Bp its bound"""
    q, eps, c = _ld(q), _ld(eps), _ld(c)
    if drift == 0:
        return np.zeros_like(p1)
    s = abs(round_to(drift, dtype)) * (1 if eps is None else np.abs(eps)) * (1 if c is None else c * c)
    return gamma_n(4, unit(dtype)) * (np.abs(q) + s * (np.abs(p1) + Bp)) + s * Bp + gamma_n(5, UO) * (np.abs(q) + s * np.abs(p1))


def energy_bound(p1, Bp, c, dtype, E1):
    c = _ld(c)
    N = p1.size
    E = 16 if dtype in (torch.float32, np.float32) else 8
    nchunks = -(-N // (256 * E))
    nblocks = min(nchunks, 1024)
    n64 = 6 + -(-nchunks // max(nblocks, 1)) + 3 + -(-nblocks // 64) + 6
    gT = gamma_n(E + 2, unit(dtype))
    c2 = 1 if c is None else c * c
    ap = np.abs(p1)
    no = 128 + int(math.ceil(math.log2(max(N, 2)))) + 3
    return float((gT + gamma_n(n64, 2.0 ** -53) * (1 + gT)) * (c2 * (ap + Bp) ** 2).sum() / 2
                 + (c2 * (2 * ap * Bp + Bp * Bp)).sum() / 2 + gamma_n(no, UO) * abs(E1))


def ratio(err, B):
    """worst |err| / B; an element whose bound is zero must be exact"""
    err, B = np.abs(np.asarray(err, dtype=np.longdouble)), np.asarray(B, dtype=np.longdouble)
    if bool(((B == 0) & (err > 0)).any()):
        return float('inf')
    return float((err / np.maximum(B, np.longdouble(1e-300))).max()) if err.size else 0.0


# ------------------------------------------------------------------------------------- restatement of leapfrog and of a move
def _each(x, fn, *others):
    """fn over the entries of a dict (or on the array itself)"""
    if isinstance(x, dict):
        return {k: fn(x[k], *[o[k] if isinstance(o, dict) else o for o in others]) for k in x}
    return fn(x, *others)


def oracle_leapfrog(q, p, grad, eps, N, cov=None, states=None):
    """
    N leapfrog steps in float64 numpy, in the reference's operation order: half kick, N - 1 x (drift, gradient, full kick),
    drift, gradient, half kick.  q, p: arrays or dicts of arrays (not modified); grad(q) -> (U, gradient) in the same
    container; eps, cov: numbers, arrays or dicts of those (cov: diagonal Cholesky factor of the covariance, None: identity).
    Returns (q, p, U at the end).
    """
    cov = 1.0 if cov is None else cov
    drift = lambda q, p, e, c: q + e * (c * (c * p))
    kick = lambda p, g, e, f: p - (f * e) * g
    U, g = grad(q)
    if states is not None:
        states.append((q, p))
    p = _each(p, kick, g, eps, 0.5)
    for i in range(N):
        q = _each(q, drift, p, eps, cov)
        U, g = grad(q)
        if i != N - 1:
            p = _each(p, kick, g, eps, 1.0)
            if states is not None:
                states.append((q, _each(p, lambda p, g, e: p + (0.5 * e) * g, g, eps)))
    p = _each(p, kick, g, eps, 0.5)
    if states is not None:
        states.append((q, p))
    return q, p, U


def chain_potential(a):
    """grad(q) -> (U, gradient dict) of the fixtures' potential for the per-key coefficients a (dict of numpy arrays)"""
    def grad(q):
        U, g = 0.0, {}
        for k in q:
            Uk, g[k] = grad_U(a[k], q[k])
            U = U + Uk
        return U, g
    return grad


class OracleHMC:
    """one chain in float64 numpy: the algorithm of sampler.HMC restated without the package"""

    def __init__(self, a, x0, eps, cov, hess, Nstep, dHmax, draws):
        self.grad, self.x, self.eps, self.cov, self.hess = chain_potential(a), dict(x0), dict(eps), cov, hess
        self.Nstep, self.dHmax, self.draws, self.ndrawn = Nstep, dHmax, draws, 0
        self.logdetM = sum(2 * np.log(hess[k]).sum() for k in hess)
        self.chain, self.Uchain = [], []
        self.U = self.grad(self.x)[0]

    def K(self, p):
        return sum(((self.cov[k] * p[k]) ** 2).sum() / 2 for k in p) + self.logdetM

    def append_chain(self):
        """what sampler.sample does after every move"""
        self.chain.append(dict(self.x))
        self.Uchain.append(self.U)

    def step(self):
        p = {k: self.hess[k] * self.draws[k][self.ndrawn] for k in self.x}
        self.ndrawn += 1
        K_start = self.K(p)
        U_start = self.grad(self.x)[0]
        H_start = K_start + U_start
        q, p, U_end = oracle_leapfrog(self.x, p, self.grad, self.eps, self.Nstep, self.cov)
        H_end = self.K(p) + U_end
        self.U = U_end
        rec = dict(K_start=K_start, H_end=H_end, p=p, u=np.nan, div=False)
        if H_end - H_start > self.dHmax:
            if len(self.Uchain) > 0:
                i = np.random.randint(0, len(self.Uchain))
                self.U, self.x = self.Uchain[i], dict(self.chain[i])
            accept, prob, rec['div'] = False, 0.0, True
        else:
            prob = min(math.exp(H_start - H_end), 1.0)
            rec['u'] = np.random.rand()
            accept = bool(np.isfinite(H_end) and rec['u'] < prob)
            if accept:
                self.x = q
            else:
                self.U = U_start
        rec.update(accept=accept, prob=prob, U=self.U, x=dict(self.x), dH=H_end - H_start)
        return rec

    def dual_averaging(self, Nadapt, target=0.8, gamma=0.05, t0=10.0, kappa=0.75):
        mu = {k: math.log(10 * self.eps[k]) for k in self.eps}
        h_bar = 0.0
        for i in range(1, Nadapt + 1):
            rec = self.step()
            eta = 1.0 / (i + t0)
            h_bar = (1 - eta) * h_bar + eta * (target - rec['prob'])
            self.eps = {k: math.exp(mu[k] - h_bar * math.sqrt(i) / gamma) for k in mu}


def chain_inputs(g):
    """(a, x0, cov, hess, draws) of the recorded chains as dicts of float64 numpy arrays"""
    ks = CHAIN['keys']
    get = lambda name: {k: g['chain_%s_%s' % (name, k)] for k in ks}
    return get('a'), get('x0'), get('cov'), get('hess'), get('draws')


def dual_eps0():
    return {k: CHAIN['dual_scale'] * v for k, v in CHAIN['eps'].items()}


def run_oracle_chain(g, tag):
    a, x0, cov, hess, draws = chain_inputs(g)
    np.random.seed(CHAIN['seed'])
    h = OracleHMC(a, x0, CHAIN['eps'], cov, hess, CHAIN['Nstep'], CHAIN['dHmax_' + tag], draws)
    recs = []
    for _ in range(CHAIN['steps']):
        recs.append(h.step())
        h.append_chain()
    return recs


def chain_discrepancy(recs, g, tag):
    """
    Largest relative discrepancy of the per-move records `recs` (dicts with prob, U, x, p, K_start, H_end, accept, div) against
    the recorded chain `tag`, each quantity relative to its largest recorded magnitude; the decisions must be equal.
    """
    pre = 'chain_%s_' % tag
    assert [bool(r['accept']) for r in recs] == g[pre + 'accept'].astype(bool).tolist(), ([r['accept'] for r in recs], g[pre + 'accept'])
    assert [bool(r['div']) for r in recs] == g[pre + 'div'].astype(bool).tolist()
    worst = 0.0
    for name in ('prob', 'U', 'K_start', 'H_end'):
        ref = g[pre + name]
        got = np.array([float(r[name]) for r in recs])
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    for name in ('x', 'p'):
        for k in CHAIN['keys']:
            ref = g[pre + name + '_' + k]
            got = np.stack([np.asarray(r[name][k]) for r in recs])
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    return worst


def leap_inputs(g, name):
    """(container, keys, q0, p0, a, eps, cov) of a leapfrog case, dicts of numpy arrays by key; eps a float for 'scalar'"""
    cont, keys, kind, with_cov = LEAP_CASES[name]
    get = lambda what: {k: g['leap_%s_%s_%s' % (name, what, k)] for k in keys}
    eps = EPS_SCALAR if kind == 'scalar' else get('eps')
    return cont, keys, get('q0'), get('p0'), get('a'), eps, (get('cov') if with_cov else None)
