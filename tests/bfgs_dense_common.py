"""
Shared by tests/test_bfgs_dense_host.py, tests/test_bfgs_dense_gpu.py and tests/golden/make_golden_bfgs_dense.py: the fixture
loader of tests/golden/bfgs_dense.npz, the case tables the generator and the tests walk together, the quadratic of the
trajectory fixtures, a plain float64 CPU oracle of the two kernel operations of csrc/bfgs.hip written as explicit sums,

    matvec:  r[i][c] = sum_j H[i][j] x[j][c]
    rank2:   H[i][j] + a (x_i z_j + z_i x_j) + b x_i x_j

the accuracy bounds the GPU tests assert, and HostBFGS: bfgs.BFGS running on that oracle.  The oracle runs on the ROUNDED
operands (H, x, z as the kernel sees them) with a and b in float64.

Bounds, with u = 2^-24 (float32) or 2^-53 (float64), gamma_n(u) = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1), derived from the order include/rime_hip.h documents:

 * matvec.  With W = 16 / sizeof(T), lane l of a wave runs one chain of fused multiply-adds over its columns
   64 W q + W l ... + W - 1, q = 0, 1, ...: lane 0 has the most, W ceil(N / (64 W)), one rounding each (columns at or beyond N
   enter as fma(0, 0, acc), exact).  The 64 chains are added by a butterfly of 6 additions.  So a term passes at most
   W ceil(N / (64 W)) + 6 roundings.  It also passes at most N: an operation rounds only when it joins a non-empty sum to a new
   term or to another non-empty sum, and a sum of N terms has N such joins (the first product included) whatever the order.
       |r - r64| <= gamma_n(u) sum_j |H_ij| |x_j|,   n = min(W ceil(N / (64 W)) + 6, N)                         matvec_bound()
   which is never looser than the recursive-summation bound gamma_N(u).
 * rank2.  H_ij passes the 2 fused multiply-adds; a term a x_i z_j the rounding of a to T, its product, the sum of the two
   products and the 2 fused multiply-adds: 5; the term b x_i x_j the rounding of b, the product and 1 fused multiply-add: 3.
   n = 6 covers all:
       |H' - H'64| <= gamma_6(u) (|H_ij| + |a| (|x_i z_j| + |z_i x_j|) + |b| |x_i x_j|)                          rank2_bound()
Nothing here is fitted to what the kernels return.

Recorded constants (measured against the REFERENCE's recorded outputs, never against the GPU code; the tests assert at
FACTOR = 100 times them, the margin of lbfgs_common: the expanded update and V^T H V differ by rounding only, amplified by the
conditioning of the problem):
 * DENSE_RESTATEMENT: the largest relative discrepancy max|r - r_ref| / max|r_ref| of a float64 CPU run of bfgs.BFGS.step on
   this file's oracle (HostBFGS) against the recorded reference trajectories, over the losses per step, the final parameters,
   the final H and the lists of s, y, alpha, Hy and the final gradient, of all four trajectories; and of implicit_to_dense
   through HostBFGS against its four records.
 * FACTORED_RESTATEMENT: the same for bfgs.factor_pairs (u, v of both FactoredInvHessian records and of the synthetic cases)
   and for the compact recurrences (bfgs.forward_shell / reverse_shell fed with numpy Gram matrices) against the recorded
   hvp, lvp and to_dense of both records.
 * FACTORED_VS_BFGS: the largest relative difference between the REFERENCE's FactoredInvHessian.to_dense() (rank2) and the
   reference's final BFGS.H of the same run, as recorded.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bfgs_dense.npz')
_CACHE = {}

FACTOR = 100.0
# measured 2026-10-20 (x86-64 CPU, numpy / torch float64) against tests/golden/bfgs_dense.npz; set by the fixed-step trajectory
# from the dense H0 (the other three: 9.4e-15, 9.7e-15, 1.2e-14; implicit_to_dense: 4.3e-15); every integer record was equal
DENSE_RESTATEMENT = 5.25e-14
# measured 2026-10-20, the same way; set by hvp / lvp / to_dense of the rank-two record (rank one: 2.7e-15; factor_pairs: 1.5e-16)
FACTORED_RESTATEMENT = 3.59e-15
# recorded 2026-10-20 by tests/golden/make_golden_bfgs_dense.py from the reference's two outputs
FACTORED_VS_BFGS = 4.89e-15

DENSE = dict(N=97, cond=1.5, max_iter=4, steps=3)
DENSE_KINDS = ('wolfe', 'fixed')                    # line_search_fn = 'strong_wolfe' | None
DENSE_H0S = ('scalar', 'dense')                     # H0 = 1.0 | diag(1 / diag(icov)) as a dense matrix
FACTORED_RUN = ('wolfe', 'scalar')                  # the trajectory whose lists feed FactoredInvHessian and implicit_to_dense
FACTORED_KINDS = ('rank2', 'rank1')
ITD_H0S = ('none', 'scalar', 'diag', 'dense')       # implicit_to_dense starting matrices
ITD_SCALAR = 0.6
# synthetic factor_pairs cases: (seed, rank2, pos, with Hy, flip the sign of y); the flipped ones return spd = False
PAIR_CASES = ((1, True, True, True, False), (2, True, False, False, False), (3, False, True, True, False),
              (4, False, False, True, False), (5, True, True, True, True))
PAIR_N = 23


def golden():
    """bfgs_dense.npz as a dict of torch tensors, loaded once and never modified by a test"""
    if GOLDEN not in _CACHE:
        with np.load(GOLDEN) as f:
            _CACHE[GOLDEN] = {k: torch.as_tensor(f[k]) for k in f.files}
    return _CACHE[GOLDEN]


def dense_cases():
    return [(kind, h0) for kind in DENSE_KINDS for h0 in DENSE_H0S]


def triu(H):
    iu = torch.triu_indices(H.shape[0], H.shape[1])
    return H[iu[0], iu[1]]


def from_triu(t, N):
    H = torch.zeros(N, N, dtype=t.dtype)
    iu = torch.triu_indices(N, N)
    H[iu[0], iu[1]] = t
    return H + H.T - torch.diag(H.diagonal())


def dense_problem(g):
    """(icov, x0) of the trajectory fixtures: loss = x^T icov x / 2"""
    return from_triu(g['dense_icov_triu'], DENSE['N']), g['dense_x0']


def dense_H0(icov, h0):
    return torch.tensor(1.0, dtype=torch.float64) if h0 == 'scalar' else torch.diag(1.0 / icov.diagonal())


def pair_inputs(case):
    """(s, y, g, alpha, Hy) of a synthetic factor_pairs case: y = A s and Hy = H y for a positive diagonal A = H^-1 plus noise"""
    seed, rank2, pos, with_Hy, flip = case
    rng = np.random.default_rng(1000 + seed)
    A = rng.uniform(0.5, 2.0, PAIR_N)
    s = rng.normal(size=PAIR_N)
    y = A * s * (-1.0 if flip else 1.0)
    alpha = float(rng.uniform(0.3, 1.5))
    g = -(rng.uniform(0.4, 2.5, PAIR_N) * s) / alpha
    Hy = y / rng.uniform(0.5, 2.0, PAIR_N)
    T = lambda a: torch.as_tensor(a, dtype=torch.float64)
    return T(s), T(y), T(g), alpha, (T(Hy) if with_Hy else None)


def recording(cls):
    """cls with a log of the accepted pairs: (s, y, alpha, the cached _Hy = H_{k+1} y_k, H_k y_k taken before the update)"""

    class Recording(cls):
        def update_hessian(self, s, y, alpha=None, **kwargs):
            if not hasattr(self, 'log'):
                self.log = []
            pre = self.hvp(y)
            out = super().update_hessian(s, y, alpha, **kwargs)
            if self._s is s:
                self.log.append((s, y, alpha, self._Hy, pre))
            return out

    return Recording


def run_dense(BFGS, icov, x0, H0, kind, device='cpu'):
    """DENSE['steps'] calls of step() of the optimiser class BFGS (store_Hy=True) on the quadratic, H0 handed over as it is (on
    the CPU: the caller's own tensor); returns what the fixture records and the optimiser.  The objective is evaluated on a float64 CPU copy of the parameters wherever these live."""
    x = x0.clone().to(device).requires_grad_(True)
    opt = recording(BFGS)((x,), H0=H0.to(device), max_iter=DENSE['max_iter'], store_Hy=True,
                          line_search_fn='strong_wolfe' if kind == 'wolfe' else None)
    opt.log = []

    def closure():
        xc = x.detach().cpu().clone().requires_grad_(True)
        loss = 0.5 * (xc @ (icov @ xc))
        loss.backward()
        x.grad = xc.grad.to(device)
        return loss.detach()

    losses = [float(opt.step(closure)) for _ in range(DENSE['steps'])]
    c = lambda t: t.detach().cpu().to(torch.float64)
    N = DENSE['N']
    stack = lambda i: torch.stack([c(e[i]) for e in opt.log]) if opt.log else torch.zeros(0, N, dtype=torch.float64)
    res = dict(losses=torch.tensor(losses, dtype=torch.float64), x=c(x), H_triu=triu(c(opt.H)), s=stack(0), y=stack(1),
               alpha=torch.tensor([float(e[2]) for e in opt.log], dtype=torch.float64), Hy=stack(3), Hy_pre=stack(4),
               g_end=c(opt._flat_grad), ints=torch.tensor([opt._exit, opt.func_evals, opt.n_iter, len(opt.log)]))
    return res, opt


def dense_discrepancy(res, g, kind, h0):
    """largest relative discrepancy of a run against the recorded trajectory; the integers must be equal"""
    key = 'dense_%s_%s_' % (kind, h0)
    assert res['ints'].tolist() == g[key + 'ints'].tolist(), (res['ints'].tolist(), g[key + 'ints'].tolist())
    worst = 0.0
    for k in ('losses', 'x', 'H_triu', 's', 'y', 'alpha', 'Hy', 'g_end'):
        ref = g[key + k]
        assert res[k].shape == ref.shape, (k, res[k].shape, ref.shape)
        worst = max(worst, rel(res[k], ref))
    return worst


def rel(r, ref):
    return float((r - ref).abs().max() / ref.abs().max())


def factored_lists(g):
    """(s, y, g_end, alpha, Hy as BFGS caches it, H_k y_k) of the trajectory FACTORED_RUN, as lists of float64 CPU tensors"""
    key = 'dense_%s_%s_' % FACTORED_RUN
    return (list(g[key + 's']), list(g[key + 'y']), g[key + 'g_end'], g[key + 'alpha'].tolist(), list(g[key + 'Hy']),
            list(g[key + 'Hy_pre']))


def factored_args(g, kind):
    """the arguments of FactoredInvHessian for a FACTORED_KINDS entry: the rank-one form needs H_k y_k"""
    s, y, g_end, alpha, Hy, Hy_pre = factored_lists(g)
    return dict(s=s, y=y, g_end=g_end, alpha=alpha, Hy=Hy if kind == 'rank2' else Hy_pre, rank2=kind == 'rank2')


def itd_H0(g, h0):
    icov, _ = dense_problem(g)
    return {'none': None, 'scalar': torch.tensor(ITD_SCALAR, dtype=torch.float64), 'diag': 1.0 / icov.diagonal(),
            'dense': torch.diag(1.0 / icov.diagonal())}[h0]


# -------------------------------------------------------------------------------------------------------------------- oracle
def _w(t):
    return torch.as_tensor(t).detach().cpu().to(torch.float64)


def oracle_matvec(H, x):
    """r[i][c] = sum_j H[i][j] x[j][c] in float64; x (N,) or (N, 2)"""
    H, x = _w(H), _w(x)
    if x.ndim == 1:
        return (H * x[None, :]).sum(1)
    return torch.stack([(H * x[None, :, c]).sum(1) for c in range(x.shape[1])], dim=1)


def oracle_matvec_abs(H, x):
    return oracle_matvec(_w(H).abs(), _w(x).abs())


def oracle_rank2(H, x, z, a, b):
    H, x, z = _w(H), _w(x), _w(z)
    return H + float(a) * (x[:, None] * z[None, :] + z[:, None] * x[None, :]) + float(b) * (x[:, None] * x[None, :])


def oracle_rank2_abs(H, x, z, a, b):
    return oracle_rank2(_w(H).abs(), _w(x).abs(), _w(z).abs(), abs(float(a)), abs(float(b)))


def unit(dtype):
    return 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53


def gamma_n(n, u):
    return n * u / (1 - n * u)


def matvec_roundings(N, dtype):
    W = 4 if dtype == torch.float32 else 2
    return min(W * -(-N // (64 * W)) + 6, N)


def matvec_bound(N, dtype, sums_abs):
    return gamma_n(matvec_roundings(N, dtype), unit(dtype)) * sums_abs


def rank2_bound(dtype, H_abs):
    return gamma_n(6, unit(dtype)) * H_abs


def ratio(err, B):
    """worst err / B; an element whose bound is zero (an exactly zero sum) must be exact"""
    err, B = err.abs(), torch.as_tensor(B)
    if bool(((B == 0) & (err > 0)).any()):
        return float('inf')
    return float((err / B.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------- the restatement on the CPU
class OracleDense:
    """bfgs._Dense with the two passes replaced by the float64 oracle above (CPU tensors)"""

    def __init__(self, N, dtype, device):
        self.N, self.dtype, self.device = N, dtype, device

    def matvec(self, H, x):
        return oracle_matvec(H, x).to(x.dtype)

    def rank2(self, H, x, z, a, b):
        H.copy_(oracle_rank2(H, x, z, a, b).to(H.dtype))
        return H


def host_bfgs():
    """bfgs.BFGS running on OracleDense: the restated algorithm without the kernels"""
    from bayeslim_amd import bfgs

    class HostBFGS(bfgs.BFGS):
        _dense_cls = OracleDense

    return HostBFGS


COV_SIZES = (5, 7)                                  # the two parameter groups of the lbfgs_approx_cov problem


def quadratic_logprob(device):
    """(an optim.LogProb whose loss is a convex quadratic of two parameter groups 'a' and 'b', both main parameters, their sizes)"""
    from bayeslim_amd import optim, dataset, utils
    na, nb = COV_SIZES
    rng = np.random.default_rng(7)
    A = torch.as_tensor(rng.normal(size=(2 * (na + nb), na + nb)) + 2.0 * np.eye(2 * (na + nb), na + nb)).to(device)

    class Quad(utils.Module):
        def __init__(self):
            super().__init__(name='quad')
            self.a = torch.nn.Parameter(torch.linspace(-1.0, 1.0, na, dtype=torch.float64, device=device))
            self.b = torch.nn.Parameter(torch.linspace(0.5, 2.0, nb, dtype=torch.float64, device=device))

        def forward(self, inp=None, prior_cache=None, **kw):
            td = dataset.TensorData()
            td.data = A @ torch.cat([self.a, self.b])
            return td

    td = dataset.TensorData()
    td.data = torch.zeros(2 * (na + nb), dtype=torch.float64, device=device)
    prob = optim.LogProb(Quad(), dataset.Dataset([td]), complex_circular=False, device=device)
    prob.set_main_params(['a', 'b'])
    return prob, COV_SIZES


def hdiag_by_hand(LBFGS, device, Nsteps, max_iter):
    """what lbfgs_approx_cov has to return on quadratic_logprob, spelled out: group 'a' alone, then group 'b' alone (from where
    the first run left the parameters), each Nsteps calls of step(); the concatenated _Hdiag"""
    prob, _ = quadratic_logprob(device)
    diags = []
    for name in ('a', 'b'):
        prob.set_main_params()
        prob.unset_param(prob.named_params)
        prob.set_main_params([name])
        opt = LBFGS((prob.main_params,), update_Hdiag=True, max_iter=max_iter)
        for _ in range(Nsteps):
            opt.step(prob.closure)
        diags.append(opt._Hdiag)
    return torch.cat(diags)


def host_shells(vec, M, u, v, both):
    """the compact form of the shell chains on the CPU: numpy Gram matrix, bfgs.forward_shell / reverse_shell, float64 sums;
    M None, a 1-d or a 2-d tensor"""
    from bayeslim_amd import bfgs
    U, V = np.stack([_w(t).numpy() for t in u]), np.stack([_w(t).numpy() for t in v])
    G = V @ U.T                                              # G[k, j] = v_k . u_j
    x = _w(vec).numpy().copy()
    if both:
        x = x + bfgs.reverse_shell(G, U @ x) @ V
    if M is not None:
        M = _w(M).numpy()
        x = M * x if M.ndim == 1 else M @ x
    return torch.as_tensor(x + bfgs.forward_shell(G, V @ x) @ U)


def host_to_dense(M, u, v, hess):
    """the dense H (the replay of FactoredInvHessian.to_dense on the oracle) or the dense L (the compact lvp of the unit vectors)"""
    N = len(u[0])
    if not hess:
        eye = torch.eye(N, dtype=torch.float64)
        return torch.stack([host_shells(eye[:, i], M, u, v, False) for i in range(N)], dim=1)
    H = torch.eye(N, dtype=torch.float64) if M is None else (torch.diag(_w(M)) if _w(M).ndim == 1 else _w(M).clone())
    dense = OracleDense(N, torch.float64, 'cpu')
    for u_k, v_k in zip(u, v):
        z = dense.matvec(H, v_k)
        dense.rank2(H, u_k, z, 1.0, float(v_k @ z))
    return H
