"""
Shared by tests/test_lm_host.py, tests/test_lm_gpu.py and tests/golden/make_golden_lm.py: the fixture loader of
tests/golden/lm.npz, the case tables the generator and the tests walk together, a plain-torch float64 CPU oracle of the
operation of rime_lm_apply written as an explicit einsum over explicit tables,

    y[o, r, i] = post[r] * sum_{k < K} M[r, k] * pre[k] * x[o, idx[k], i]                  x [O, K_in, I],  y [O, R, I]

and the accuracy bound the GPU tests assert.  The oracle runs on the ROUNDED operands (x, M, pre, post as the kernel sees them).

Bound, for every output element, with u = 2^-24 (f32) or 2^-53 (f64) and gamma_n = n u / (1 - n u):

    |y - y64| <= f gamma_n |post[r]| sum_k |M[r, k]| |pre[k]| |x[o, idx[k], i]|

Derivation (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a recursively accumulated inner product in
which each partial result is rounded once has every term multiplied by at most n factors (1 + delta), |delta| <= u).
 * x or M real (real . real, complex . real, real . complex): the real part and the imaginary part of an output are each ONE
   chain of K fused multiply-adds, one rounding each; before it every input is scaled by pre (one rounding) and after it the
   sum by post (one rounding).  A term meets at most K + 2 roundings: n = K + 2.  The two parts have the errors
   e_re <= gamma_n sum |M| |x_re| and e_im <= gamma_n sum |M| |x_im| (the complex factor split in its parts), and
   sqrt(e_re^2 + e_im^2) <= gamma_n sum |M| |x| by the triangle inequality in the plane: f = 1.
 * x and M complex: a part is one chain of 2 K fused multiply-adds (re: Mr xr - Mi xi, im: Mr xi + Mi xr): n = 2 K + 2.  With
   a, b = |Mr|, |Mi| and c, d = |xr|, |xi| the parts of one term are bounded by a c + b d and a d + b c, and
   (a c + b d)^2 + (a d + b c)^2 = (a^2 + b^2)(c^2 + d^2) + 4 a b c d <= 2 |M|^2 |x|^2: f = sqrt(2).  With out_real only the
   real part is formed; a c + b d <= sqrt(2) |M| |x| holds as well, so the same n and f apply.
 * the scatter of a backward pass through idx adds the m results that share an input (index_add_): m - 1 more roundings,
   n grows by m - 1 (m the largest multiplicity in idx).
Nothing here is fitted to what the kernel returns.

least_squares in float32 is compared with the float64 evaluation of xhat = D z, z = A^H (Ninv y), on the same f32-rounded A, y,
Ninv AND the D the call returned (D is the small torch-side matrix; its own rounding is torch's and is checked in float64
only).  Margin: |D| Bz + gamma_{K+1} |D| |z64|, with Bz the bound above for z (n one larger when Ninv weights y, for that
product's rounding) and the second term the K-term application of D: ls_margin().

The float32 normal matrix and its inverse are checked on their own, D32 against D64 = (A^H N^-1 A + eps I)^-1 formed in float64
from the same rounded A and Ninv: d_margin().  The float32 normal matrix carries an elementwise error E <= gamma_{Ns+2}
|A|^H |N^-1| |A| (an Ns-term sum, the weight's product, eps); a perturbation E of a matrix moves its inverse by at most
||D||^2 ||E|| / (1 - ||D|| ||E||) (Higham, section 14.1: (B + E)^-1 - B^-1 = -B^-1 E (B + E)^-1); and a backward
stable inversion of a K x K matrix in float32 (LU, or the eigen / singular value decomposition behind pinv) adds a forward
error of at most p(K) u kappa ||D|| with p a polynomial of low degree, taken as 4 K^2.  In the spectral norm (E's bounded by its
Frobenius norm):  ||D32 - D64||_2 <= ||D||^2 ||E||_F / (1 - ||D|| ||E||_F) + 4 K^2 u kappa_2 ||D||_2.
mode='lstsq' (torch.linalg.lstsq, a QR solve) in float32 against the float64 solution of the same rounded problem, per data
column b with solution x and residual r: ||x32 - x||_2 <= 4 Ns K u (kappa ||x|| + kappa^2 ||r|| / ||A||), the first-order
perturbation bound of a least-squares problem (Higham, theorem 20.1) for a backward error of Ns K u, doubled twice for the
higher-order terms and the constant of the Householder analysis: lstsq_margin().
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lm.npz')
MINI = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rime_lm_mini.npz')
_CACHE = {}

BASES = ('direct', 'legendre', 'chebyshevt', 'chebyshevu', 'laguerre')
NDEGS = (1, 4, 9)
XNAMES = ('nonuni', 'uni')
# option sets of the extra gen_poly_A fixtures poly_opt_<name>: legendre, Ndeg 4, the non-uniform samples
POLY_OPTS = {'logx': dict(logx=True, whiten=True), 'd0': dict(d0=1.25, whiten=False), 'x0dx': dict(whiten=True, x0=1.1, dx=0.9),
             'qr': dict(qr=True, whiten=True), 'logx_d0': dict(logx=True, d0=0.5, whiten=False)}
PREP_OPTS = {'plain': dict(), 'd0': dict(d0=2.0), 'logx': dict(logx=True), 'whiten': dict(whiten=True),
             'all': dict(d0=2.0, logx=True, whiten=True), 'x0dx': dict(whiten=True, x0=1.0, dx=0.75)}
FOURIER = ((None, 'ortho'), (None, 'backward'), (5, 'ortho'), (5, 'backward'))

NS = 6                                   # samples of every custom A of the forward fixtures
FWD_SHAPE = (2, 3, 4, 5)
# LinearModel.forward fixtures fwd_<i>: input fwd_xr / fwd_xc (FWD_SHAPE), or their [0, 0, :, 0] line for one=True; custom A
# fwd_Ar_<K> / fwd_Ac_<K> (NS, K); coeff 'vec' (along dim) / 'full' (FWD_SHAPE); idx = (L - 1, 0, 0) of an axis of length L
FWD_CASES = (
    dict(dim=0), dict(dim=1), dict(dim=-2), dict(dim=-1), dict(dim=0, one=True),
    dict(dim=0, xc=True, ac=True), dict(dim=1, xc=True), dict(dim=-2, ac=True), dict(dim=-1, xc=True, ac=True),
    dict(dim=-1, ac=True, one=True),
    dict(dim=1, coeff='vec'), dict(dim=-1, coeff='vec', xc=True, ac=True), dict(dim=-2, coeff='full'),
    dict(dim=-2, idx=True), dict(dim=-1, idx=True, coeff='vec', xc=True), dict(dim=1, idx=True, ac=True),
    dict(dim=1, diag=True), dict(dim=3, diag=True, xc=True),
    dict(dim=-2, xc=True, ac=True, out_real=True), dict(dim=-1, ac=True, out_real=True), dict(dim=1, xc=True, out_real=True),
    dict(dim=-2, out_dtype='complex128'), dict(dim=1, xc=True, ac=True, out_real=True, out_dtype='complex128'),
    dict(dim=-2, out_reshape=(2, 3, NS * 5)), dict(dim=0, xc=True, out_reshape=(-1,)),
)
# least_squares fixtures ls_<i>: A ls_Ar / ls_Ac (NS, 3) along dim 1 of y ls_yr / ls_yc (2, NS, 5); Ninv 'vec' (NS,) / 'full'
LS_CASES = (
    dict(norm=None), dict(norm='inv'), dict(norm='pinv'), dict(norm='diag'), dict(norm='inv', pinv=False, eps=0.1),
    dict(norm='pinv', eps=0.05, rcond=1e-12, hermitian=False), dict(norm='inv', Ninv='vec'), dict(norm='diag', Ninv='vec'),
    dict(norm='diag', Ninv='full'), dict(norm=None, Ninv='vec'), dict(mode='lstsq'), dict(mode='lstsq', Ninv='vec'),
    dict(norm='pinv', ac=True), dict(norm='diag', ac=True, Ninv='vec'), dict(norm='chol', eps=0.01), dict(norm='chol', Ninv='vec'),
)

# kernel cases of the GPU tests: strided (O, K, R, I), last-axis (O, K, R)
STRIDED = ((1, 1, 1, 3), (3, 2, 7, 65), (1, 5, 70, 64), (2, 32, 33, 130), (2, 33, 32, 130), (1, 33, 70, 67), (3, 70, 5, 257),
           (1, 8, 256, 300))
LAST = ((1, 1, 1), (5, 3, 64), (67, 6, 65), (3, 40, 130), (130, 130, 7))
# (x complex, M complex, out_real)
COMBOS = ((False, False, False), (True, False, False), (False, True, False), (True, True, False), (True, True, True))


def golden(path=None):
    """lm.npz (or rime_lm_mini.npz) as a dict of torch tensors, loaded once and never modified by a test"""
    path = GOLDEN if path is None else path
    if path not in _CACHE:
        with np.load(path) as f:
            _CACHE[path] = {k: torch.as_tensor(f[k]) for k in f.files}
    return _CACHE[path]


def unit(dtype):
    return 2.0 ** -24 if dtype in (torch.float32, torch.complex64) else 2.0 ** -53


def _wide(t):
    t = torch.as_tensor(t)
    if not (t.requires_grad and t.device.type == 'cpu'):          # a CPU leaf keeps its graph: the oracle's own autograd
        t = t.detach()
    t = t.cpu()
    return t.to(torch.complex128) if t.is_complex() else t.to(torch.float64)


def oracle(x, M, idx=None, pre=None, post=None, out_real=False):
    """the operation of the module docstring in float64 on the CPU; x [O, K_in, I], M [R, K]"""
    x, M = _wide(x), _wide(M)
    if idx is not None:
        x = x[:, torch.as_tensor(idx).cpu().long(), :]
    if pre is not None:
        x = x * _wide(pre)[None, :, None]
    if x.is_complex() != M.is_complex():
        x, M = x.to(torch.complex128), M.to(torch.complex128)
    y = torch.einsum('rk,oki->ori', M, x)
    if post is not None:
        y = y * _wide(post)[None, :, None]
    return y.real if (out_real and y.is_complex()) else y


def gamma(n, dtype):
    u = unit(dtype)
    return n * u / (1 - n * u)


def bound(x, M, dtype, idx=None, pre=None, post=None, extra=0):
    """the bound of the module docstring, [O, R, I] float64; `extra` further roundings per term"""
    x, M = _wide(x), _wide(M)
    both = x.is_complex() and M.is_complex()
    K = M.shape[1]
    n, f = (2 * K + 2, np.sqrt(2.0)) if both else (K + 2, 1.0)
    xa = x.abs()
    if idx is not None:
        xa = xa[:, torch.as_tensor(idx).cpu().long(), :]
    if pre is not None:
        xa = xa * _wide(pre).abs()[None, :, None]
    S = torch.einsum('rk,oki->ori', M.abs(), xa)
    if post is not None:
        S = S * _wide(post).abs()[None, :, None]
    return f * gamma(n + extra, dtype) * S


def ratio(y, y64, B):
    """worst |y - y64| / B; an element whose bound is zero (an exactly zero sum) must be exact"""
    err = (_wide(y).detach() - y64.detach()).abs()
    if bool(((B == 0) & (err > 0)).any()):
        return float('inf')
    return float((err / B.clamp_min(1e-300)).max())


def ls_margin(D, Bz, z64, dim, dtype):
    """|D| Bz + gamma_{K+1} |D| |z64| along axis dim (module docstring)"""
    Da = _wide(D).abs()
    app = lambda t: torch.movedim(torch.tensordot(t, Da, dims=([dim], [1])), -1, dim)
    return app(Bz) + gamma(Da.shape[1] + 1, dtype) * app(z64.abs())


def d_margin(A, Ninv, D64, dtype):
    """the bound on ||D32 - D64||_2 of the module docstring; A (Ns, K), Ninv (Ns,) or None, as rounded"""
    Aa = _wide(A).abs()
    w = torch.ones(Aa.shape[0], dtype=torch.float64) if Ninv is None else _wide(Ninv).abs()
    E = float((gamma(Aa.shape[0] + 2, dtype) * (Aa.T @ (w[:, None] * Aa))).norm())
    sv = torch.linalg.svdvals(_wide(D64))
    nD, kappa, K = float(sv[0]), float(sv[0] / sv[-1]), Aa.shape[1]
    return nD ** 2 * E / (1 - nD * E) + 4 * K ** 2 * unit(dtype) * kappa * nD


def lstsq_margin(A, x64, r64, dtype):
    """the bound on the 2-norm of the float32 error of every column of a least-squares solution; x64 (K, Nb), r64 (Ns, Nb)"""
    sv = torch.linalg.svdvals(_wide(A))
    kappa, Ns, K = float(sv[0] / sv[-1]), A.shape[0], A.shape[1]
    return 4 * Ns * K * unit(dtype) * (kappa * x64.norm(dim=0) + kappa ** 2 * r64.norm(dim=0) / float(sv[0]))


def rand(rng, shape, cplx, dtype=torch.float64):
    v = rng.normal(size=shape)
    if cplx:
        v = v + 1j * rng.normal(size=shape)
        return torch.as_tensor(v).to(torch.complex64 if dtype == torch.float32 else torch.complex128)
    return torch.as_tensor(v).to(dtype)


def idx_for(L):
    """the gather of the fixtures along an axis of length L: a repeated entry, and omitted ones when L > 2"""
    return torch.as_tensor([L - 1, 0, 0])


def fwd_setup(g, case):
    """(params, A, coeff, idx, d) of forward fixture `case` from the golden dict g, float64 / complex128 on the CPU"""
    c = dict(case)
    x = g['fwd_xc'] if c.get('xc') else g['fwd_xr']
    if c.get('one'):
        x = x[0, 0, :, 0].clone()
    d = 0 if x.ndim == 1 else c['dim'] % x.ndim
    L = x.shape[d]
    idx = idx_for(L) if c.get('idx') else None
    K = 3 if idx is not None else L
    if c.get('diag'):
        A = (g['fwd_Ac_%d' % K] if c.get('ac') else g['fwd_Ar_%d' % K])[:K, :K].clone()
    else:
        A = g['fwd_Ac_%d' % K] if c.get('ac') else g['fwd_Ar_%d' % K]
    coeff = None
    if c.get('coeff') == 'vec':
        coeff = g['fwd_coeff_%d' % L]
        if d != x.ndim - 1:
            coeff = coeff.reshape([-1 if a == d else 1 for a in range(x.ndim)])
    elif c.get('coeff') == 'full':
        coeff = g['fwd_coeff_full']
    return x, A, coeff, idx, d


def fwd_model(lm_module, A, coeff, idx, case, dim):
    """LinearModel('custom') of a forward fixture from module `lm_module` (the product's or the reference's)"""
    odt = getattr(torch, case['out_dtype']) if case.get('out_dtype') else None
    return lm_module.LinearModel('custom', A=A, dim=dim, coeff=coeff, idx=idx, diag=bool(case.get('diag')), out_dtype=odt,
                                 out_reshape=case.get('out_reshape'), out_real=bool(case.get('out_real')))


def fwd_oracle(x, A, coeff, idx, d, case):
    """LinearModel.forward of a non-diag fixture through oracle(): any coeff multiplied first, the axis moved to [O, K, I]"""
    x = _wide(x)
    if coeff is not None:
        x = x * _wide(coeff)
    shape = tuple(x.shape)
    O, I = int(np.prod(shape[:d], dtype=np.int64)), int(np.prod(shape[d + 1:], dtype=np.int64))
    y = oracle(x.reshape(O, shape[d], I), A, idx=idx, out_real=bool(case.get('out_real')))
    y = y.reshape(shape[:d] + (y.shape[1],) + shape[d + 1:])
    if case.get('out_dtype') and not case.get('out_real'):
        y = y.to(getattr(torch, case['out_dtype']))
    if case.get('out_reshape'):
        y = y.reshape(case['out_reshape'])
    return y


def ls_setup(g, case):
    cplx = bool(case.get('ac'))
    A, y = (g['ls_Ac'], g['ls_yc']) if cplx else (g['ls_Ar'], g['ls_yr'])
    Ninv = {'vec': g['ls_Ninv_vec'], 'full': g['ls_Ninv_full'], None: None}[case.get('Ninv')]
    kw = {k: v for k, v in case.items() if k not in ('ac', 'Ninv')}
    return A, y, Ninv, kw
