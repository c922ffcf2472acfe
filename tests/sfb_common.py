"""
Shared by tests/test_sfb_host.py and tests/test_sfb_gpu.py: the float64 CPU oracle of the SFB radial transform (a plain torch
restatement of the per-degree products a_lm(r) = sum_n g_l(k_ln r) t_lmn, held to tests/golden/sfb.npz in test_sfb_host.py)
and the unpacking of the fixture's concatenated per-degree arrays.
"""
import numpy as np
import torch


def oracle(params, mats, col_lists, Nr, Nlm):
    """params (..., Nlmn) float64 / complex128 on the CPU -> (..., Nr, Nlm): per degree, (Nk, Nr)^T @ (Nk, Nl) into its columns"""
    params = torch.as_tensor(params)
    assert params.dtype in (torch.float64, torch.complex128) and not params.is_cuda
    out = torch.zeros(params.shape[:-1] + (Nr, Nlm), dtype=params.dtype)
    off = 0
    for G, cols in zip(mats, col_lists):
        G = torch.as_tensor(G, dtype=torch.float64).to(params.dtype)
        Nk, Nl = G.shape[0], len(cols)
        p = params[..., off:off + Nk * Nl].reshape(params.shape[:-1] + (Nk, Nl))
        out[..., torch.as_tensor(np.asarray(cols, dtype=np.int64))] = G.T @ p
        off += Nk * Nl
    assert off == params.shape[-1]
    return out


def oracle_grad(params, w, mats, col_lists, Nr, Nlm):
    """(out, d Re sum(conj(w) out) / d params) by autograd through the oracle"""
    p = torch.as_tensor(params).clone().requires_grad_(True)
    out = oracle(p, mats, col_lists, Nr, Nlm)
    w = torch.as_tensor(w)
    ((out * w.conj()).real.sum() if out.is_complex() else (out * w).sum()).backward()
    return out.detach(), p.grad.detach()


def unpack_basis(g, tag):
    """(keys, kln dict, gln dict of float64 (Nk, Nr) tensors, column lists) of the `tag` ('shell' | 'ball') basis of sfb.npz"""
    keys = [int(k) for k in g[tag + '_keys']]
    nk, nl = g[tag + '_nk'], g[tag + '_nl']
    ks = np.split(g[tag + '_kln'], np.cumsum(nk)[:-1])
    Gs = np.split(g[tag + '_gln'], np.cumsum(nk)[:-1])
    cs = np.split(g[tag + '_alm_idx'], np.cumsum(nl)[:-1])
    kln = {k: v for k, v in zip(keys, ks)}
    gln = {k: torch.as_tensor(v) for k, v in zip(keys, Gs)}
    return keys, kln, gln, [c.astype(np.int64) for c in cs]


def relmax(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return np.abs(a - b).max() / np.abs(b).max()
