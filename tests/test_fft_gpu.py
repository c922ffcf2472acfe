"""
GPU checks of the fused FFT kernel (csrc/fft.hip) through ops.fft_apply and bayeslim_amd/fft.py against the float64 CPU
oracle of tests/fft_common.py, which runs on the ROUNDED operands (the data and the window as the kernel sees them).

Bound, per line and for every output element:  |y - y64| <= B = u (2 + sopfr(N)) s sqrt(N) ||w o x||_2  (fft_common),
abs: B, square: B (2 |y64| + B), peaknorm: 2 B / (m - B).  The adjoint (the backward pass) is the same transform of the
cotangent c with the window on the store; the windows of these tests lie in (0, 1], so its bound is B with ||c||_2.
PeakDelay: 1e-4 df in float32, 1e-9 df in float64.  Every test prints its worst error / bound ratio before it asserts.

Measured on an MI355X (worst error / bound over all cases of this file): see DESIGN.md, "Fourier layer".
"""
import numpy as np
import pytest
import torch

import fft_common as fc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RDT = {'f32': torch.float32, 'f64': torch.float64}
CDT = {'f32': torch.complex64, 'f64': torch.complex128}


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def plan_for(N, prec):
    from bayeslim_amd import ops
    return ops.FFTPlan(N, RDT[prec], DEV)


def ratio(y, y64, B):
    return float(((y.detach().cpu().to(y64.dtype) - y64).abs() / B).max())


def line_cases(N):
    """(shape, ifft, shift, window, norm): 1, 3 and 150 lines (several work-groups plus a tail), 1000 lines for N <= 8 (many
    lines per work-group); both directions, both shifts, window and none and the three norms meet every N"""
    cases = [((N,), False, True, True, None),
             ((3, N), True, True, False, 'ortho'),
             ((1, 1, 30, 5, N), False, False, True, 'forward'),
             ((2, N), True, False, True, 'backward')]
    if N <= 8:
        cases.append(((1000, N), False, True, False, None))
    return cases


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('N', fc.SIZES)
def test_forward_and_backward_against_the_oracle(N, prec):
    from bayeslim_amd import ops
    rng = np.random.default_rng(1000 + N)
    plan = plan_for(N, prec)
    worst = 0.0
    for shape, ifft, shift, use_win, norm in line_cases(N):
        x = fc.tone_input(rng, shape, cdtype=CDT[prec])
        c = fc.tone_input(rng, shape, amp=0.0, cdtype=CDT[prec])
        w = fc.window_vec(rng, N).to(RDT[prec]) if use_win else None
        xg = x.to(DEV).requires_grad_(True)
        y = ops.fft_apply(xg, plan, inverse=ifft, window=None if w is None else w.to(DEV), shift=shift, norm=norm)
        gx, = torch.autograd.grad(y, xg, c.to(DEV))
        assert y.shape == x.shape and y.dtype == CDT[prec] and gx.shape == x.shape and gx.dtype == CDT[prec]
        y64 = fc.oracle_linear(x, ifft=ifft, win=w, fftshift=shift, norm=norm)
        g64 = fc.oracle_adjoint(c, ifft=ifft, win=w, fftshift=shift, norm=norm)
        rf = ratio(y, y64, fc.bound(x, N, RDT[prec], ifft=ifft, win=w, norm=norm))
        rb = ratio(gx, g64, fc.bound(c, N, RDT[prec], ifft=ifft, win=None, norm=norm))
        print('RATIO linear N %d %s lines %d ifft %d shift %d win %d norm %s: fwd %.3f bwd %.3f' % (
            N, prec, x.numel() // N, ifft, shift, use_win, norm, rf, rb))
        worst = max(worst, rf, rb)
    assert worst <= 1.0, worst


@pytest.mark.parametrize('N', [30, 37, 130, 256])
def test_adjoint_identity(N):
    """<y, A x> = <A^H y, x> in float64, A with window, shift and norm, A^H as autograd runs it"""
    from bayeslim_amd import ops
    rng = np.random.default_rng(N)
    plan = plan_for(N, 'f64')
    for ifft, shift in ((False, True), (True, True), (False, False)):
        x = fc.tone_input(rng, (5, N)).to(DEV).requires_grad_(True)
        yv = fc.tone_input(rng, (5, N), amp=0.0).to(DEV)
        w = fc.window_vec(rng, N).to(DEV)
        Ax = ops.fft_apply(x, plan, inverse=ifft, window=w, shift=shift, norm='ortho')
        AHy, = torch.autograd.grad(Ax, x, yv)
        lhs, rhs = torch.vdot(yv.reshape(-1), Ax.detach().reshape(-1)), torch.vdot(AHy.reshape(-1), x.detach().reshape(-1))
        rel = float((lhs - rhs).abs() / lhs.abs())
        print('RATIO adjoint N %d ifft %d shift %d: %.2e' % (N, ifft, shift, rel))
        assert rel < 1e-12


COMBOS = [(True, False, False), (False, False, True), (False, True, False), (True, True, False), (True, False, True),
          (False, True, True), (True, True, True)]


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('N', [8, 37, 256, 1000])
def test_epilogues_fused_and_through_torch(N, prec):
    """every combination of abs / peaknorm / square: fused in the kernel under no_grad, and as torch expressions on the
    kernel's spectrum when a gradient is asked for; both within the derived bound of the float64 chain"""
    from bayeslim_amd import ops
    rng = np.random.default_rng(77 + N)
    plan = plan_for(N, prec)
    x = fc.tone_input(rng, (7, N), cdtype=CDT[prec])
    w = fc.window_vec(rng, N).to(RDT[prec])
    xd, wd = x.to(DEV), w.to(DEV)
    y64 = fc.oracle_linear(x, win=w, fftshift=True)
    B = fc.bound(x, N, RDT[prec], win=w)
    worst = 0.0
    for ab, pn, sq in COMBOS:
        name = '+'.join(n for n, on in (('abs', ab), ('peaknorm', pn), ('square', sq)) if on)
        z64 = fc.chain(y64, abs=ab, peaknorm=pn, square=sq)
        Bz = fc.epilogue_bound(B, y64, abs=ab, peaknorm=pn, square=sq)
        with torch.no_grad():
            zf = ops.fft_apply(xd, plan, window=wd, shift=True, epilogue=name)
        zn = ops.fft_apply(xd, plan, window=wd, shift=True, epilogue=name)            # no gradient asked for: fused too
        assert torch.equal(zf, zn) and not zf.requires_grad
        xg = xd.clone().requires_grad_(True)
        zt = ops.fft_apply(xg, plan, window=wd, shift=True, epilogue=name)
        assert zt.requires_grad and zt.dtype == zf.dtype == (RDT[prec] if (ab or sq) else CDT[prec]) and zt.shape == zf.shape
        r1, r2 = ratio(zf, z64, Bz), ratio(zt, z64, Bz)
        print('RATIO epilogue N %d %s %s: fused %.3f torch %.3f' % (N, prec, name, r1, r2))
        worst = max(worst, r1, r2)
        g, = torch.autograd.grad(zt.abs().sum() if zt.is_complex() else zt.sum(), xg)
        assert bool(torch.isfinite(torch.view_as_real(g)).all())
    assert worst <= 1.0, worst
    # gradient of sum c |y|^2 = A^H (2 c y): the error of y (<= B) through A^H (norm s sqrt(N) max w, w <= 1) plus the
    # adjoint's own bound on its input 2 c y
    c = torch.as_tensor(rng.uniform(0.5, 1.5, (7, N))).to(RDT[prec])
    xg = xd.clone().requires_grad_(True)
    g, = torch.autograd.grad((ops.fft_apply(xg, plan, window=wd, shift=True, epilogue='square') * c.to(DEV)).sum(), xg)
    cot = 2 * c.double() * y64
    g64 = fc.oracle_adjoint(cot, win=w, fftshift=True)
    Bg = np.sqrt(N) * torch.sqrt(((2 * c.double() * B) ** 2).sum(-1, keepdim=True)) + fc.bound(cot, N, RDT[prec])
    rg = ratio(g, g64, Bg)
    print('RATIO epilogue N %d %s square gradient: %.3f' % (N, prec, rg))
    assert rg <= 1.0


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_other_axes_and_real_input(prec):
    from bayeslim_amd import ops
    rng = np.random.default_rng(3)
    for shape, dim in (((30, 3, 5), 0), ((2, 37, 3), 1), ((4, 5, 64), -1)):
        N = shape[dim]
        plan = plan_for(N, prec)
        x = fc.tone_input(rng, shape[:dim] + shape[dim:][1:] + (N,), cdtype=CDT[prec]).movedim(-1, dim).contiguous()
        c = fc.tone_input(rng, shape, amp=0.0, cdtype=CDT[prec])
        xg = x.to(DEV).requires_grad_(True)
        y = ops.fft_apply(xg, plan, dim=dim, shift=True)
        gx, = torch.autograd.grad(y, xg, c.to(DEV))
        assert y.shape == x.shape and gx.shape == x.shape
        rf = ratio(y, fc.oracle_linear(x, dim=dim, fftshift=True), fc.bound(x, N, RDT[prec], dim=dim))
        rb = ratio(gx, fc.oracle_adjoint(c, dim=dim, fftshift=True), fc.bound(c, N, RDT[prec], dim=dim))
        print('RATIO dim %d N %d %s: fwd %.3f bwd %.3f' % (dim, N, prec, rf, rb))
        assert max(rf, rb) <= 1.0
    # a real input is promoted to complex; its gradient is real
    N = 97
    plan = plan_for(N, prec)
    x = torch.as_tensor(rng.normal(size=(3, N))).to(RDT[prec])
    c = fc.tone_input(rng, (3, N), amp=0.0, cdtype=CDT[prec])
    xg = x.to(DEV).requires_grad_(True)
    y = ops.fft_apply(xg, plan, inverse=True, shift=True)
    gx, = torch.autograd.grad(y, xg, c.to(DEV))
    assert y.dtype == CDT[prec] and gx.dtype == RDT[prec]
    rf = ratio(y, fc.oracle_linear(x, ifft=True, fftshift=True), fc.bound(x, N, RDT[prec], ifft=True))
    rb = ratio(gx, fc.oracle_adjoint(c, ifft=True, fftshift=True).real, fc.bound(c, N, RDT[prec], ifft=True))
    print('RATIO real input N %d %s: fwd %.3f bwd %.3f' % (N, prec, rf, rb))
    assert max(rf, rb) <= 1.0
    with pytest.raises(TypeError):
        ops.fft_apply(xg.to(torch.float64 if prec == 'f32' else torch.float32), plan)
    with pytest.raises(ValueError):
        ops.fft_apply(xg[:, :50], plan)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('N', [64, 97, 256])
def test_peak_delay_against_the_oracle(N, prec):
    """tones at fractional bins plus 1 % noise: a unique maximum and positive arguments of Quinn's logarithms"""
    from bayeslim_amd import fft
    old = torch.get_default_dtype()
    torch.set_default_dtype(RDT[prec])
    try:
        rng = np.random.default_rng(N)
        tones = np.array([3.3, 9.71, N / 2 + 0.48, N - 6.88, N - 1.1, 0.25])
        x = np.exp(2j * np.pi * tones[:, None] * np.arange(N) / N) + 0.01 * (rng.normal(size=(6, N)) + 1j * rng.normal(size=(6, N)))
        x = torch.as_tensor(x).reshape(2, 3, N).to(CDT[prec])
        tol = (1e-4 if prec == 'f32' else 1e-9)
        worst = 0.0
        for kw in fc.PEAK_CASES:
            F = fft.PeakDelay(dim=2, N=N, ndim=3, dx=0.25, **kw)
            out = F(x.to(DEV))
            assert out.shape == (2, 3, 1) and out.dtype == RDT[prec] and not out.requires_grad
            win = None if F.win is None else F.win.to(RDT[prec])
            z64 = fc.oracle(x, dim=2, win=win, fftshift=F.fftshift, abs=F.abs, peaknorm=F.peaknorm, square=F.square)
            ref = fc.oracle_peak(z64, float(F.start), float(F.df))
            err = float((out.cpu().double()[..., 0] - ref).abs().max()) / float(F.df)
            print('RATIO peak N %d %s %s: error %.3e df (bound %.0e df)' % (N, prec, kw, err, tol))
            worst = max(worst, err)
        assert worst <= tol, worst
    finally:
        torch.set_default_dtype(old)


def test_peak_delay_against_the_reference(f64):
    from bayeslim_amd import fft
    g = fc.golden()
    for i, kw in enumerate(fc.PEAK_CASES):
        F = fft.PeakDelay(dim=2, N=32, ndim=3, dx=0.25, device=DEV, **kw)
        out = F(g['peak_x'].to(DEV))
        err = float((out.cpu() - g['peak_%d' % i]).abs().max()) / float(F.df)
        print('RATIO peak golden case %d: error %.3e df' % (i, err))
        assert out.shape == g['peak_%d' % i].shape and err <= 1e-9


@pytest.mark.parametrize('case', range(len(fc.FWD_CASES)))
def test_fft_object_against_the_reference(f64, case):
    from bayeslim_amd import fft
    g = fc.golden()
    kw, dim = fc.FWD_CASES[case]
    x = g['fwd_x'] if dim in (-1, 2) else g['fwd_x'].movedim(-1, dim).contiguous()
    F = fft.FFT(dim=dim, N=12, ndim=3, dx=0.5, **kw)
    y = F(x.to(DEV))
    ref = g['fwd_%d' % case]
    y64 = fc.oracle_linear(x, dim=dim, ifft=F.ifft, win=F.win, fftshift=F.fftshift, norm=F.norm)
    B = fc.bound(x, 12, torch.float64, ifft=F.ifft, win=F.win, norm=F.norm, dim=dim)
    Bz = fc.epilogue_bound(B, y64, dim=dim, abs=F.abs, peaknorm=F.peaknorm, square=F.square)
    assert y.shape == ref.shape and y.dtype == ref.dtype
    r = ratio(y, ref, Bz)
    print('RATIO golden forward case %d: %.3f' % (case, r))
    assert r <= 1.0


def test_fft_object_windows_numpy_and_limits(f64):
    from bayeslim_amd import fft
    g = fc.golden()
    x = g['fwd_x']
    F = fft.FFT(dim=2, N=12, device=DEV)
    y = F(x.to(DEV), win=g['fwd_winfull'].to(DEV))                     # a window of the data's shape: multiplied in torch
    B = fc.bound(x * g['fwd_winfull'], 12, torch.float64)
    assert ratio(y, g['fwd_winfull_out'], B) <= 1.0
    y2 = F(x.numpy(), win=g['fwd_winfull'])                              # numpy in: moved to the object's device
    assert y2.is_cuda and torch.equal(y2, y)
    yi = F(x.to(DEV), ifft=True)
    assert ratio(yi, fc.oracle_linear(x, ifft=True, fftshift=True), fc.bound(x, 12, torch.float64, ifft=True)) <= 1.0
    F32 = fft.FFT(dim=1, ndim=2, N=16, window='hann', device=DEV)
    F32.push(torch.float32)
    assert F32.win.dtype == torch.float32 and F32.win.is_cuda
    with pytest.raises(ValueError, match='4096'):
        fft.FFT(dim=0)(torch.zeros(4097, dtype=torch.complex64, device=DEV))


@pytest.mark.parametrize('N,epilogue', [(256, 'abs'), (37, 'peaknorm'), (1000, 'none'), (64, 'peak')])
def test_two_runs_are_bit_identical(N, epilogue):
    from bayeslim_amd import ops
    rng = np.random.default_rng(9)
    plan = plan_for(N, 'f32')
    x = fc.tone_input(rng, (1, 1, 30, 5, N), cdtype=torch.complex64).to(DEV)
    w = fc.window_vec(rng, N).float().to(DEV)
    with torch.no_grad():
        a = ops.fft_apply(x, plan, window=w, shift=True, epilogue=epilogue)
        b = ops.fft_apply(x, plan, window=w, shift=True, epilogue=epilogue)
    assert torch.equal(a, b)
    xg = x.clone().requires_grad_(True)
    ga, = torch.autograd.grad(ops.fft_apply(xg, plan, window=w, shift=True), xg, x)
    gb, = torch.autograd.grad(ops.fft_apply(xg, plan, window=w, shift=True), xg, x)
    assert torch.equal(ga, gb)


def test_fft_of_a_visdata_and_vis_wedge(f64):
    from bayeslim_amd import fft
    g = fc.golden()
    vd = fc.hex7_visdata(g, device=DEV)
    d0 = vd.data.clone()
    F = fft.FFT(dim=4, ndim=5, N=vd.Nfreqs, dx=float(vd.freqs[1] - vd.freqs[0]), window='bh')
    out = F(vd)
    assert out is not vd and torch.equal(vd.data, d0) and np.array_equal(out.blnums, vd.blnums)
    x = g['hex_data']
    win = F.win.reshape(-1)
    assert ratio(out.data, fc.oracle_linear(x, win=win, fftshift=True), fc.bound(x, 12, torch.float64, win=win)) <= 1.0
    wv, FT = fft.vis_wedge(vd, window='bh', abs=True)
    assert isinstance(FT, fft.FFT) and np.array_equal(np.asarray(wv.bls), g['wedge_bls'].numpy())
    assert float((FT.freqs - g['wedge_delays']).abs().max()) <= 1e-12 * float(g['wedge_delays'].abs().max())
    assert float((FT.win.reshape(-1).cpu() - g['wedge_win']).abs().max()) <= 1e-12
    xa = g['blavg_data']
    r = ratio(wv.data, g['wedge_data'], fc.bound(xa, 12, torch.float64, win=g['wedge_win']))
    print('RATIO vis_wedge: %.3f' % r)
    assert wv.data.shape == g['wedge_data'].shape and wv.data.dtype == torch.float64 and r <= 1.0
    # float32 data, window kept in the default dtype: the kernel takes it in the precision of the data
    vd32 = fc.hex7_visdata(g, device=DEV, dtype=torch.complex64)
    w32, _ = fft.vis_wedge(vd32, window='bh', abs=True)
    xa32 = vd32.bl_average().data.cpu()
    z64 = fc.oracle(xa32, win=g['wedge_win'].float(), fftshift=True, abs=True)
    assert w32.data.dtype == torch.float32
    assert ratio(w32.data, z64, fc.bound(xa32, 12, torch.float32, win=g['wedge_win'].float())) <= 1.0


def test_profile_tuples():
    """ops.PROFILE receives one ('fft_kernel', start, end, lines x N) per launch: the forward, then the backward"""
    from bayeslim_amd import ops
    rng = np.random.default_rng(5)
    x = torch.as_tensor(rng.normal(size=(3, 8)) + 1j * rng.normal(size=(3, 8))).to(torch.complex64).to(DEV).requires_grad_(True)
    plan = plan_for(8, 'f32')
    prof = []
    ops.PROFILE = prof
    try:
        y = ops.fft_apply(x, plan)
        assert len(prof) == 1
        y.abs().sum().backward()
    finally:
        ops.PROFILE = None
    torch.cuda.synchronize()
    assert len(prof) == 2 and all(len(k) == 4 and k[0] == 'fft_kernel' and k[3] == 24 for k in prof), prof
    assert all(k[1].elapsed_time(k[2]) >= 0 for k in prof)
    ops.fft_apply(x.detach(), plan)
    assert len(prof) == 2                                      # nothing is recorded once PROFILE is None again
