#!/usr/bin/env python3
"""
Golden vectors of the filter layer (reference filt.py): every covariance builder on a short axis, GPFilter's G and V for the
'pinv' and 'chol' inversions, invert_matrix in its other modes, and outputs + the gradient of sum |y|^2 with respect to the
input of MatFilter (real and complex G, residual on and off, a rectangular G, in-painting with input_idx, dim = -2) and of
WedgeFilter on a tensor and on a VisData (two filters, one real and one complex, interleaved baselines, two baselines in no
group).  TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes tests/golden/filt.npz, arrays
only, everything float64 / complex128.

Finding (reference): MatFilter.setup_filter and LstSqFilter.setup_filter name an undefined `device` (filt.py:87, 349) and
raise NameError when given a G; the fixtures build filters through the constructors.
Finding (reference): WedgeFilter on a VisData copies the data detached (VisData.copy(copydata=True), dataset.py:556), so no
gradient reaches the input on that route; `wedge_grad` comes from the tensor route on the same data, `wedge_out_vd` is
asserted equal to `wedge_out` here.
Finding (reference): under torch 2.10 MatFilter.predict raises on a real G with complex data (einsum of Double with
ComplexDouble, filt.py:121).  The real-G cases are therefore the reference run on the real and on the imaginary part of the
data, recombined (y = G xr + i G xi; the gradient of sum |y|^2 likewise), and the real member of the wedge is handed to
the reference typed complex with a zero imaginary part.
Finding (reference): gauss_sinc_cov(high_prec=False) calls torch.special.erf on a complex tensor, which torch does not
implement; only high_prec=True is pinned.

Usage:  python tests/golden/make_golden_filt.py
"""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


def run(filt, x):
    """output and d sum|y|^2 / dx of a reference filter on a tensor"""
    x = x.clone().requires_grad_(True)
    y = filt(x)
    (y.abs() ** 2).sum().backward()
    return y.detach(), x.grad.detach()


def run_parts(make, x):
    """a real-G filter on complex data: the reference on the real and the imaginary part, recombined"""
    yr, gr = run(make(), x.real)
    yi, gi = run(make(), x.imag)
    return torch.complex(yr, yi), torch.complex(gr, gi)


def gen_filt(ba):
    ft = ba.filt
    rng = np.random.default_rng(71)
    cn = lambda *s: torch.as_tensor(rng.normal(size=s) + 1j * rng.normal(size=s))
    out = {}

    # builders: 12 samples, and 7 prediction points for the non-square forms
    x = torch.linspace(0.0, 1.1, 12)
    x2 = torch.linspace(0.05, 0.95, 7)
    out.update(bx=x, bx2=x2)
    out['rbf'] = ft.rbf_cov(x, 0.3, amp=2.0)
    out['rbf_x2'] = ft.rbf_cov(x, 0.3, x2=x2)
    out['exp'] = ft.exp_cov(x, 0.4, amp=1.5)
    out['exp_x2'] = ft.exp_cov(x, 0.4, x2=x2)
    out['sinc'] = ft.sinc_cov(x, 0.25)
    out['sinc_x2'] = ft.sinc_cov(x, 0.25, x2=x2)
    out['phasor'] = ft.phasor_mat(x, 1.7)
    out['phasor_pos_x2'] = ft.phasor_mat(x, 1.7, neg=False, x2=x2)
    out['gauss_sinc'] = ft.gauss_sinc_cov(x, 0.5, 0.3)
    out['gauss_sinc_x2'] = ft.gauss_sinc_cov(x, 0.5, 0.3, x2=x2)
    A, ev = ft.gen_cov_modes(out['rbf'], N=4)
    out.update(modes_N4=A, modes_evals=ev)
    A, _ = ft.gen_cov_modes(out['rbf'], rcond=1e-6)
    out['modes_rcond'] = A

    # GPFilter G, V
    Cs, Cn = ft.sinc_cov(x, 0.4), torch.eye(12) * 1e-3
    for inv in ('pinv', 'chol'):
        gp = ft.GPFilter(Cs.clone(), Cn.clone(), inv=inv, rcond=1e-12)
        out.update({'gp_G_' + inv: gp.G, 'gp_V_' + inv: gp.V})
    out.update(gp_Cs=Cs, gp_Cn=Cn)
    C = Cs + Cn
    for inv, kw in (('inv', {}), ('diag', {}), ('pinv', dict(rcond=1e-8, hermitian=True)), ('chol', dict(eps=1e-2))):
        out['inv_' + inv] = ba.linalg.invert_matrix(C.clone(), inv=inv, **kw)
    out['inv_C'] = C

    # MatFilter on tensors: N = 16 samples
    N = 16
    f = torch.linspace(0.0, 1.0, N)
    Greal = ft.GPFilter(ft.sinc_cov(f, 0.3), torch.eye(N) * 1e-2).G
    Gcplx = (ft.GPFilter(ft.sinc_cov(f, 0.3) * ft.phasor_mat(f, 2.0), torch.eye(N) * 1e-2, hermitian=True).G).to(torch.complex128)
    xin = cn(2, 3, N)
    out.update(mat_x=xin, mat_G_real=Greal, mat_G_cplx=Gcplx)
    for tag, G in (('real', Greal), ('cplx', Gcplx)):
        for res in (0, 1):
            y, g = (run_parts(lambda: ft.MatFilter(G, residual=bool(res)), xin) if tag == 'real'
                    else run(ft.MatFilter(G, residual=bool(res)), xin))
            out.update({'mat_%s_res%d_out' % (tag, res): y, 'mat_%s_res%d_grad' % (tag, res): g})
    # rectangular: 9 prediction points from 16 samples
    f9 = torch.linspace(0.1, 0.9, 9)
    Cx = ft.sinc_cov(f, 0.3, x2=f9)
    Grect = ft.GPFilter(ft.sinc_cov(f, 0.3), torch.eye(N) * 1e-2, Cs_cross=Cx, Cs_pred=ft.sinc_cov(f9, 0.3)).G
    assert tuple(Grect.shape) == (9, N)
    y, g = run_parts(lambda: ft.MatFilter(Grect), xin)
    out.update(rect_G=Grect, rect_out=y, rect_grad=g)
    # in-painting: samples idx predicted from the OTHER samples (their columns of G are zero), written into idx
    idx = torch.as_tensor([2, 3, 7, 11, 15])
    keep = np.setdiff1d(np.arange(N), idx.numpy())
    Gin = torch.zeros(len(idx), N)
    Gin[:, keep] = ft.GPFilter(ft.sinc_cov(f[keep], 0.3), torch.eye(len(keep)) * 1e-2, Cs_cross=ft.sinc_cov(f[keep], 0.3, x2=f[idx]),
                               Cs_pred=ft.sinc_cov(f[idx], 0.3)).G
    out.update(inp_G=Gin, inp_idx=idx)
    for res in (0, 1):
        y, g = run_parts(lambda: ft.MatFilter(Gin, residual=bool(res), input_idx=idx), xin)
        out.update({'inp_res%d_out' % res: y, 'inp_res%d_grad' % res: g})
    mask = torch.zeros(N, dtype=bool)
    mask[idx] = True
    y, _ = run_parts(lambda: ft.MatFilter(Gin, input_idx=mask), xin)
    assert torch.equal(y, out['inp_res0_out'])
    # dim = -2
    xd = cn(2, N, 3)
    y, g = run(ft.MatFilter(Gcplx, dim=-2, residual=True), xd)
    out.update(dim2_x=xd, dim2_out=y, dim2_grad=g)

    # WedgeFilter: 7 baselines, filter 0 (real G) on three of them, filter 1 (complex G) on two, two in no group
    bls = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 4)]
    filt2bls = {0: [(0, 1), (1, 2), (0, 4)], 1: [(0, 3), (2, 3)]}
    xv = cn(1, 1, len(bls), 2, N)
    mk = lambda: [ft.MatFilter(Greal.to(torch.complex128), residual=True), ft.MatFilter(Gcplx, residual=True)]
    wf = ft.WedgeFilter(mk(), filt2bls, bls=bls)
    y, g = run(wf, xv)
    out.update(wedge_x=xv, wedge_bls=np.asarray(bls), wedge_out=y, wedge_grad=g,
               wedge_bls0=np.asarray(filt2bls[0]), wedge_bls1=np.asarray(filt2bls[1]))
    vd = ba.dataset.VisData()
    vd.setup_data(bls, np.array([2459861.0, 2459861.1]), f * 1e8 + 1e8, pol='ee', data=xv.clone())
    yv = ft.WedgeFilter(mk(), filt2bls)(vd).data
    assert torch.equal(yv, y)
    out['wedge_out_vd'] = yv
    out.update(wedge_times=np.array([2459861.0, 2459861.1]), wedge_freqs=f * 1e8 + 1e8)
    mg.save('filt', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    ba = mg.bootstrap_reference()
    ba.filt = importlib.import_module('bayeslim.filt')
    gen_filt(ba)
