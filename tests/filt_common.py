"""
Shared by tests/test_filt_host.py and tests/test_filt_gpu.py: the fixture loader of tests/golden/filt.npz and a float64 CPU
oracle of the operation of rime_filt_apply, written as a plain einsum over explicit tables:

    acc[l, i]   = sum_k W[f(l)][i, k] x[l, ic[k]]
    y[l, oc[i]] = s acc[l, i] + base[i] x[l, oc[i]]          lines with f(l) = -1 are copied

`apply_tables` runs it for given tables, `oracle_filter` builds forward and adjoint from ops.filt_tables (the tables the
product uses) for a tensor of lines (..., Nbl, inner, N) and returns y, the adjoint applied to a cotangent, and the
per-element error scale  sum_k |W_ik| |x_k| + base_i |x_i|  of both.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'filt.npz')
_CACHE = {}


def golden():
    """filt.npz as a dict of float64 / complex128 / integer torch tensors, loaded once and never modified by a test"""
    if 'g' not in _CACHE:
        with np.load(GOLDEN) as f:
            _CACHE['g'] = {k: torch.as_tensor(f[k]) for k in f.files}
    return _CACHE['g']


def apply_tables(x, W, line_filt, ic, oc, base, s, Ny, y0=None):
    """x (L, Nx) complex128, W (Nfilt, M, K), line_filt (L,) int64 -> y (L, Ny) and the error scale (L, Ny)"""
    x = x.to(torch.complex128)
    L = x.shape[0]
    ic, oc = torch.as_tensor(ic, dtype=torch.int64), torch.as_tensor(oc, dtype=torch.int64)
    base = torch.as_tensor(base, dtype=torch.float64)
    y = torch.zeros(L, Ny, dtype=torch.complex128) if y0 is None else y0.clone().to(torch.complex128)
    scale = torch.zeros(L, Ny, dtype=torch.float64)
    sel = line_filt >= 0
    if (~sel).any():
        assert x.shape[1] == Ny
        y[~sel] = x[~sel]
    if sel.any():
        Wl = W[line_filt[sel]]
        xs = x[sel]
        acc = torch.einsum('lik,lk->li', Wl.to(torch.complex128), xs[:, ic])
        keep = base[None, :] * xs[:, oc] if bool((base != 0).any()) else 0.0
        ys, sc = y[sel], scale[sel]
        ys[:, oc] = s * acc + keep
        sc[:, oc] = torch.einsum('lik,lk->li', Wl.abs().to(torch.float64), xs[:, ic].abs()) + \
            (base[None, :] * xs[:, oc].abs() if bool((base != 0).any()) else 0.0)
        y[sel], scale[sel] = ys, sc
    return y, scale


def oracle_filter(x, G, residual=False, input_idx=None, bl2filt=None, cot=None):
    """
    x (..., N) or, with bl2filt, (..., Nbl, inner, N); G (M, K) or (Nfilt, M, K).  Returns (y, scale_y, gx, scale_gx):
    gx is the adjoint applied to `cot` (None: to y itself, so that 2 gx is the gradient of sum |y|^2).
    """
    from bayeslim_amd import ops
    G = torch.as_tensor(G)
    if G.ndim == 2:
        G = G[None]
    M, K = G.shape[1:]
    tab = ops.filt_tables(M, K, residual, input_idx)
    x = torch.as_tensor(x).to(torch.complex128)
    xl = x.reshape(-1, x.shape[-1])
    if bl2filt is None:
        lf = torch.zeros(xl.shape[0], dtype=torch.int64)
    else:
        b2f = torch.as_tensor(bl2filt, dtype=torch.int64)
        lf = b2f[None, :, None].expand(xl.shape[0] // (x.shape[-3] * x.shape[-2]), x.shape[-3], x.shape[-2]).reshape(-1)
    ic, oc, base, s = tab['fwd']
    y, sy = apply_tables(xl, G, lf, ic, oc, base, s, tab['Ny'], y0=xl if tab['idx'] is not None else None)
    c = y if cot is None else torch.as_tensor(cot).to(torch.complex128).reshape(-1, tab['Ny'])
    ic, oc, base, s = tab['bwd']
    GH = G.transpose(1, 2).conj() if G.is_complex() else G.transpose(1, 2)
    gx, sg = apply_tables(c, GH, lf, ic, oc, base, s, K)
    shp = x.shape[:-1]
    return y.reshape(shp + (-1,)), sy.reshape(shp + (-1,)), gx.reshape(shp + (K,)), sg.reshape(shp + (K,))


def cnormal(rng, *shape):
    return torch.as_tensor(rng.normal(size=shape) + 1j * rng.normal(size=shape))
