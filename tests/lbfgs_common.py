"""
Shared by tests/test_lbfgs_host.py, tests/test_lbfgs_gpu.py and tests/golden/make_golden_bfgs.py: the fixture loader of
tests/golden/bfgs.npz, the case tables the generator and the tests walk together, the objectives of the line-search and
trajectory fixtures, a plain float64 CPU oracle of the two kernel operations written as explicit sums over rows,

    dots:     out[0][j] = s_j . v    out[1][j] = y_j . (d o v)    out[2][j] = s_j . y_k    out[3][j] = y_j . s_k    out[4][j] = y_j . (d o y_k)
    combine:  r = gamma * d o (v - sum_j a_j y_j) + sum_j b_j s_j

and the accuracy bounds the GPU tests assert.  The oracle runs on the ROUNDED operands (the rows, v and d as the kernel sees
them) with a, b and gamma in float64.

Bounds, with u = 2^-24 (float32) or 2^-53 (float64) for the working precision T, u64 = 2^-53, gamma_n(u) = n u / (1 - n u)
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: in a sum of products accumulated with one rounding per
step, every term is multiplied by at most as many factors (1 + delta), |delta| <= u, as there are roundings on its way):

 * dots.  A lane holds E = 64 / sizeof(T) elements of a chunk and accumulates them in ONE chain of E fused multiply-adds in
   T: E roundings.  Where d is given, d o v (or d o y_k) is formed first, one more rounding: E + 1.  The lane's sum is
   widened exactly, and everything after that is float64 additions, each value passing through at most
       n64 = 6 (butterfly of a wave) + C (chunks of a work-group, C = ceil(nchunks / nblocks)) + 3 (waves of a work-group)
             + ceil(nblocks / 64) (partials a lane of the second stage adds) + 6 (its butterfly) + 1 (the oracle's own
             float64 product d o v, which the kernel forms in T -- counted above -- but the oracle rounds to float64)
   of them, nchunks = ceil(N / (256 E)), nblocks = min(nchunks, 1024).  So
       |out - out64| <= (gamma_{E+1}(u) + gamma_{n64}(u64) (1 + gamma_{E+1}(u))) sum_e |a_e| |b_e|                  dots_bound()
   with a, b the two vectors of the product (|y| and |d| |v| for out[1], and so on).
 * combine.  Every element is one chain in T: q = v, m fused multiply-adds with -a_j (a_j rounded to T: 1), the product
   gamma * d (gamma rounded to T: 1, the product: 1), times q (1), m fused multiply-adds with b_j (rounded to T: 1).  The
   term v passes 2 m + 3 roundings, a term a_j y_j at most 1 + m + 3 + m, a term b_j s_j at most 1 + m: n = 2 m + 4 covers
   all, and
       |r - r64| <= gamma_{2m+4}(u) (|gamma| |d| (|v| + sum_j |a_j| |y_j|) + sum_j |b_j| |s_j|)                      combine_bound()
Nothing here is fitted to what the kernels return.

Recorded constants (measured against the REFERENCE's recorded outputs, never against the GPU code; the tests assert at
FACTOR = 100 times them, because the compact form and the two-loop recursion differ by rounding only, amplified by the
conditioning of the small triangular systems):
 * TLR_RESTATEMENT: the largest relative discrepancy max|r - r_ref| / max|r_ref| of bfgs.compact_coeffs fed with float64 Gram
   matrices of the fixture's s, y, vec (numpy dot products) + the float64 combine of this file, over every two_loop_recursion
   fixture.
 * TRAJ_RESTATEMENT: the largest relative discrepancy of a float64 CPU run of bfgs.LBFGS.step with this file's oracle in place
   of the kernels (HostLBFGS: compact_coeffs + torch dot products) against the recorded reference trajectories, over the
   losses per step, the final parameters, _Hdiag and _rho of both trajectories.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bfgs.npz')
_CACHE = {}

FACTOR = 100.0
# measured 2026-10-18 (x86-64 CPU, numpy / torch float64) against tests/golden/bfgs.npz; set by the case tlr_37_7_diag
# (with rho as recorded and with rho = 1 / diag(SY) alike)
TLR_RESTATEMENT = 4.47e-16
# measured 2026-10-18 (x86-64 CPU, torch float64) against tests/golden/bfgs.npz; set by the final parameters of the fixed-step
# trajectory (the strong-Wolfe one: 2.6e-15, its _rho); exit code, func_evals, n_iter and the pair count were equal
TRAJ_RESTATEMENT = 3.03e-15

# two_loop_recursion fixtures tlr_<N>_<m>_<kind>: s, y (m, N), vec (N,), rho (m,), H0 scalar TLR_SCALAR or the diagonal tlr_<N>_diag
TLR_NS, TLR_MS, TLR_KINDS = (37, 300), (1, 2, 7), ('scalar', 'diag')
TLR_SCALAR = 0.37
TLR_COMPLEX = dict(N=37, m=3)                       # tlrc_*: complex s, y, vec, a real diagonal

# cubic_interpolate fixtures: (x1, f1, g1, x2, f2, g2, bound_lo, bound_hi), nan bounds = None
CUBIC_ARGS = (
    (0.0, 1.0, -1.0, 1.0, 0.6, 0.3, np.nan, np.nan),          # interior minimum, x1 < x2
    (1.0, 0.6, 0.3, 0.0, 1.0, -1.0, np.nan, np.nan),          # the same points, x1 > x2
    (0.0, 1.0, -1.0, 1.0, 0.2, -0.5, 1.01, 10.0),             # extrapolation with bounds (bracketing phase)
    (0.0, 1.0, -1.0, 2.0, 5.0, 1.0, np.nan, np.nan),          # clipped at a bound
    (0.0, 1.0, 1.0, 1.0, 1.6, 1.0, np.nan, np.nan),           # d2_square < 0: the midpoint
    (2.0, 1.9, 1.0, 0.5, 1.0, 1.0, 0.25, 4.0),                # d2_square < 0 with bounds, x1 > x2
    (0.3, 2.0, -4.0, 0.9, 1.5, 2.5, np.nan, np.nan),
    (0.9, 1.5, 2.5, 0.3, 2.0, -4.0, 0.35, 0.85),
)

WOLFE_N = 12
TRAJ = dict(N=300, cond=1.5, history_size=5, max_iter=4, steps=3)
TRAJ_KINDS = ('wolfe', 'fixed')                     # line_search_fn = 'strong_wolfe' | None


def golden():
    """bfgs.npz as a dict of torch tensors, loaded once and never modified by a test"""
    if GOLDEN not in _CACHE:
        with np.load(GOLDEN) as f:
            _CACHE[GOLDEN] = {k: torch.as_tensor(f[k]) for k in f.files}
    return _CACHE[GOLDEN]


def tlr_cases():
    return [(N, m, kind) for N in TLR_NS for m in TLR_MS for kind in TLR_KINDS]


def tlr_inputs(g, N, m, kind):
    """(s, y, vec, rho, H0, ref) of a real fixture"""
    key = 'tlr_%d_%d' % (N, m)
    H0 = torch.tensor(TLR_SCALAR, dtype=torch.float64) if kind == 'scalar' else g['tlr_%d_diag' % N]
    return g[key + '_s'], g[key + '_y'], g[key + '_vec'], g[key + '_rho'], H0, g[key + '_%s_out' % kind]


# ---------------------------------------------------------------------------------------------------------------- objectives
def wolfe_objective(name):
    """(f, x0, p, alpha0, c2) of a line-search fixture: f maps a float64 tensor x to (loss, gradient).
    'newton': a separable quadratic along its Newton direction, the first trial alpha = 1 satisfies both conditions.
    'quartic': sum x^4 / 4 + c x^2 / 2 along a short steepest-descent direction with a tight curvature condition: the step
    grows twice (bracketing) and is then refined twice (zoom), five evaluations."""
    c = torch.linspace(0.5, 3.0, WOLFE_N, dtype=torch.float64)
    x0 = torch.linspace(-1.0, 2.0, WOLFE_N, dtype=torch.float64)
    if name == 'newton':
        def f(x):
            return 0.5 * (c * x * x).sum(), c * x
        return f, x0, -x0.clone(), 1.0, 0.9
    if name == 'quartic':
        def f(x):
            return (x ** 4 / 4 + c * x * x / 2).sum(), x ** 3 + c * x
        return f, x0, -0.02 * f(x0)[1], 1.0, 0.1
    raise NameError(name)


def wolfe_obj_func(f):
    def obj_func(x, alpha, p):
        loss, grad = f(x + alpha * p)
        return float(loss), grad
    return obj_func


def traj_problem(g):
    """(icov, x0, H0) of the trajectory fixtures: loss = x^T icov x / 2, the diagonal H0 = 1 / diag(icov)"""
    N = TRAJ['N']
    icov = torch.zeros(N, N, dtype=torch.float64)
    iu = torch.triu_indices(N, N)
    icov[iu[0], iu[1]] = g['traj_icov_triu']
    icov = icov + icov.T - torch.diag(icov.diagonal())
    return icov, g['traj_x0'], 1.0 / icov.diagonal()


def run_trajectory(LBFGS, icov, x0, H0, kind, device='cpu'):
    """TRAJ['steps'] calls of step() of the optimiser class LBFGS on the quadratic; returns a dict of what the fixture records.
    The objective and its gradient are evaluated on a float64 CPU copy of the parameters wherever these live (the same
    arithmetic for the reference, the restatement and the GPU run), so a run differs from the record through the
    optimiser's own arithmetic only."""
    x = x0.clone().to(device).requires_grad_(True)
    opt = LBFGS((x,), H0=H0.clone().to(device), history_size=TRAJ['history_size'], max_iter=TRAJ['max_iter'],
                update_Hdiag=True, line_search_fn='strong_wolfe' if kind == 'wolfe' else None)

    def closure():
        xc = x.detach().cpu().clone().requires_grad_(True)
        loss = 0.5 * (xc @ (icov @ xc))
        loss.backward()
        x.grad = xc.grad.to(device)
        return loss.detach()

    losses = [float(opt.step(closure)) for _ in range(TRAJ['steps'])]
    return dict(losses=torch.tensor(losses, dtype=torch.float64), x=x.detach().cpu(), Hdiag=opt._Hdiag.detach().cpu(),
                rho=torch.tensor([float(r) for r in opt._rho], dtype=torch.float64),
                ints=torch.tensor([opt._exit, opt.func_evals, opt.n_iter, len(opt._s)])), opt


def traj_discrepancy(res, g, kind):
    """largest relative discrepancy of a run against the recorded trajectory; the integers must be equal"""
    assert res['ints'].tolist() == g['traj_%s_ints' % kind].tolist(), (res['ints'].tolist(), g['traj_%s_ints' % kind].tolist())
    worst = 0.0
    for k in ('losses', 'x', 'Hdiag', 'rho'):
        ref = g['traj_%s_%s' % (kind, k)]
        assert res[k].shape == ref.shape, (k, res[k].shape, ref.shape)
        worst = max(worst, float((res[k] - ref).abs().max() / ref.abs().max()))
    return worst


# -------------------------------------------------------------------------------------------------------------------- oracle
def _w(t):
    return torch.as_tensor(t).detach().cpu().to(torch.float64)


def oracle_dots(S, Y, v, d=None, k=None):
    """(2 or 5, m) float64: the sums of the module docstring, row by row; S, Y sequences of real vectors"""
    v = _w(v)
    dv = v if d is None else _w(d) * v
    m = len(S)
    out = torch.zeros(2 if k is None else 5, m, dtype=torch.float64)
    if k is not None:
        sk, yk = _w(S[k]), _w(Y[k])
        dyk = yk if d is None else _w(d) * yk
    for j in range(m):
        sj, yj = _w(S[j]), _w(Y[j])
        out[0, j] = (sj * v).sum()
        out[1, j] = (yj * dv).sum()
        if k is not None:
            out[2, j] = (sj * yk).sum()
            out[3, j] = (yj * sk).sum()
            out[4, j] = (yj * dyk).sum()
    return out


def oracle_dots_abs(S, Y, v, d=None, k=None):
    """the same sums over absolute values: what the bound multiplies"""
    ab = lambda t: None if t is None else _w(t).abs()
    return oracle_dots([ab(t) for t in S], [ab(t) for t in Y], ab(v), ab(d), k)


def oracle_combine(S, Y, v, d, a, b, gamma):
    q = _w(v).clone()
    for j in range(len(Y)):
        q = q - float(a[j]) * _w(Y[j])
    r = gamma * q if d is None else gamma * _w(d) * q
    for j in range(len(S)):
        r = r + float(b[j]) * _w(S[j])
    return r


def oracle_combine_abs(S, Y, v, d, a, b, gamma):
    q = _w(v).abs()
    for j in range(len(Y)):
        q = q + abs(float(a[j])) * _w(Y[j]).abs()
    r = abs(gamma) * q if d is None else abs(gamma) * _w(d).abs() * q
    for j in range(len(S)):
        r = r + abs(float(b[j])) * _w(S[j]).abs()
    return r


def oracle_two_loop(vec, s, y, rho, gamma, d):
    """the two-loop recursion itself (Nocedal & Wright, algorithm 7.4) in float64 on real vectors"""
    q = _w(vec).clone()
    m = len(s)
    al = [0.0] * m
    for i in reversed(range(m)):
        al[i] = float(rho[i]) * float(_w(s[i]) @ q)
        q = q - al[i] * _w(y[i])
    r = gamma * q if d is None else gamma * _w(d) * q
    for i in range(m):
        be = float(rho[i]) * float(_w(y[i]) @ r)
        r = r + (al[i] - be) * _w(s[i])
    return r


def unit(dtype):
    return 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53


def gamma_n(n, u):
    return n * u / (1 - n * u)


def dots_bound(N, dtype, sums_abs):
    """the dots bound of the module docstring for the float64 sums of absolute values `sums_abs`"""
    E = 16 if dtype == torch.float32 else 8
    nchunks = -(-N // (256 * E))
    nblocks = min(nchunks, 1024)
    n64 = 6 + -(-nchunks // nblocks) + 3 + -(-nblocks // 64) + 6 + 1
    gT = gamma_n(E + 1, unit(dtype))
    return (gT + gamma_n(n64, 2.0 ** -53) * (1 + gT)) * sums_abs


def combine_bound(m, dtype, r_abs):
    return gamma_n(2 * m + 4, unit(dtype)) * r_abs


def ratio(err, B):
    """worst err / B; an element whose bound is zero (an exactly zero sum) must be exact"""
    err, B = err.abs(), torch.as_tensor(B)
    if bool(((B == 0) & (err > 0)).any()):
        return float('inf')
    return float((err / B.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------- the restatement on the CPU
class OracleHistory:
    """bfgs._History with the two passes replaced by the float64 oracle above (CPU tensors)"""

    def __init__(self, N, dtype, device, d):
        self.N, self.dtype, self.device, self.d = N, dtype, device, d
        self.s, self.y = [], []

    def set_rows(self, s, y):
        self.s, self.y = list(s), list(y)

    def dots(self, v, k=-1):
        return oracle_dots(self.s, self.y, v, self.d, None if k < 0 else k).numpy()

    def combine(self, v, a, b, gamma):
        return oracle_combine(self.s, self.y, v, self.d, a, b, gamma).to(v.dtype)


def host_lbfgs():
    """bfgs.LBFGS running on OracleHistory: the restated algorithm without the kernels"""
    from bayeslim_amd import bfgs

    class HostLBFGS(bfgs.LBFGS):
        _history_cls = OracleHistory

    return HostLBFGS


def gram(S, Y, d=None):
    """float64 Gram matrices SY[i, j] = s_i . y_j, YDY[i, j] = y_i . (d o y_j) of real rows, numpy"""
    S, Y = np.stack([_w(t).numpy() for t in S]), np.stack([_w(t).numpy() for t in Y])
    D = Y if d is None else Y * _w(d).numpy()[None]
    return S @ Y.T, Y @ D.T


def realify(t):
    """the interleaved real view of a complex tensor (a copy), a real tensor unchanged"""
    t = torch.as_tensor(t)
    return torch.view_as_real(t.contiguous()).reshape(*t.shape[:-1], -1).clone() if t.is_complex() else t
