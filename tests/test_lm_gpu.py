"""
GPU checks of the linear-model kernels (csrc/lm.hip) through ops.lm_apply, bayeslim_amd/linear_model.py and linalg.py against
the float64 CPU oracle of tests/lm_common.py, which runs on the ROUNDED operands (x, M, pre, post as the kernel sees them).

Bound, for every output element (derived in lm_common):  |y - y64| <= f gamma_n |post| sum_k |M| |pre| |x|, n = K + 2 and
f = 1 when x or M is real, n = 2 K + 2 and f = sqrt(2) when both are complex; the scatter of a backward pass through a
repeated idx adds its multiplicity - 1 to n.  Every test prints its worst error / bound ratio before it asserts.
"""
import copy
import pickle

import numpy as np
import pytest
import torch

import lm_common as lc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RDT = {'f32': torch.float32, 'f64': torch.float64}


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def operands(rng, O, K, R, I, xc, mc, dt, K_in=None):
    return lc.rand(rng, (O, K if K_in is None else K_in, I), xc, dt), lc.rand(rng, (R, K), mc, dt)


def run_case(O, K, R, I, prec, rng, with_idx=False, with_scale=False, combos=lc.COMBOS):
    """forward and transpose of one shape in the five type combinations; returns the worst error / bound"""
    from bayeslim_amd import ops
    dt = RDT[prec]
    worst = 0.0
    for xc, mc, oreal in combos:
        K_in = K + 2 if with_idx else K
        x, M = operands(rng, O, K, R, I, xc, mc, dt, K_in)
        idx = torch.as_tensor(rng.integers(0, K_in - 1, K)) if with_idx else None      # the last entry is never named
        if with_idx and K > 1:
            idx[-1] = idx[0]                                                           # a repeated entry
        coeff = torch.as_tensor(rng.uniform(0.5, 2.0, K_in)).to(dt) if with_scale else None
        pre = None if coeff is None else (coeff if idx is None else coeff[idx])
        plan = ops.LMPlan(M, idx=idx, coeff=coeff)
        y = ops.lm_apply(x.to(DEV), plan, dim=1, out_real=oreal)
        y64 = lc.oracle(x, M, idx=idx, pre=pre, out_real=oreal)
        assert y.shape == y64.shape == (O, R, I) and y.is_complex() == y64.is_complex() and lc._wide(y).dtype == y64.dtype
        rf = lc.ratio(y, y64, lc.bound(x, M, dt, idx=idx, pre=pre))
        # transpose: z = pre * (M^H c), compact; the cotangent has y's type
        c = lc.rand(rng, (O, R, I), y64.is_complex(), dt)
        planT = ops.LMPlan(M, coeff=pre)
        z = ops.lm_apply(c.to(DEV), planT, dim=1, adjoint=True, out_real=oreal)
        MH = M.conj().T.resolve_conj()
        z64 = lc.oracle(c, MH, post=pre, out_real=oreal)
        assert z.shape == z64.shape == (O, K, I) and z.is_complex() == z64.is_complex()
        rb = lc.ratio(z, z64, lc.bound(c, MH, dt, post=pre))
        print('RATIO kernel (%d,%d,%d,%d) %s xc %d mc %d real %d idx %d scale %d: fwd %.3f transpose %.3f' % (
            O, K, R, I, prec, xc, mc, oreal, with_idx, with_scale, rf, rb))
        worst = max(worst, rf, rb)
    return worst


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('shape', lc.STRIDED)
def test_strided_kernels_against_the_oracle(shape, prec):
    O, K, R, I = shape
    assert run_case(O, K, R, I, prec, np.random.default_rng(sum(shape))) <= 1.0


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('shape', lc.LAST)
def test_last_axis_kernel_against_the_oracle(shape, prec):
    O, K, R = shape
    assert run_case(O, K, R, 1, prec, np.random.default_rng(sum(shape))) <= 1.0


@pytest.mark.parametrize('shape,combos', [((1, 5, 40, 270001), lc.COMBOS[:1] + lc.COMBOS[3:4]), ((1, 5, 40, 530001), lc.COMBOS[:1] + lc.COMBOS[3:4]),
                                          ((1, 5, 33, 1100003), lc.COMBOS[:1])])
def test_strided_kernels_with_several_columns_per_lane(shape, combos):
    """the strided kernels give a lane 2 or 4 columns once the grid is large enough (lm.hip, lm_cpl): these are the smallest
    shapes that take those paths, with a column count that is no multiple of the block's.  Forward (few-in, K = 5, two row
    chunks) / transpose (few-out, 5 rows): 270 001 columns: 2 / 1 per lane; 530 001: 4 / 2; 1 100 003: 4 / 4"""
    O, K, R, I = shape
    assert run_case(O, K, R, I, 'f32', np.random.default_rng(I), with_scale=True, combos=combos) <= 1.0


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('shape', [(3, 5, 70, 65), (2, 40, 9, 33), (67, 6, 65, 1)])
def test_gather_and_scalings_against_the_oracle(shape, prec):
    O, K, R, I = shape
    rng = np.random.default_rng(7 + sum(shape))
    assert run_case(O, K, R, I, prec, rng, with_idx=True, with_scale=True) <= 1.0
    assert run_case(O, K, R, I, prec, rng, with_idx=True) <= 1.0
    assert run_case(O, K, R, I, prec, rng, with_scale=True) <= 1.0


@pytest.mark.parametrize('shape', [(3, 5, 70, 65), (2, 40, 9, 33), (67, 6, 65, 1), (3, 40, 130, 1)])
def test_adjoint_identity(shape):
    """<y, A x> = <A^H y, x> in float64 with idx and coeff, A^H as autograd runs it"""
    from bayeslim_amd import ops
    O, K, R, I = shape
    rng = np.random.default_rng(sum(shape))
    for xc, mc in ((True, True), (False, False), (True, False)):
        K_in = K + 2
        x = lc.rand(rng, (O, K_in, I), xc).to(DEV).requires_grad_(True)
        M = lc.rand(rng, (R, K), mc)
        idx = torch.as_tensor(rng.integers(0, K_in, K))
        idx[-1] = idx[0]
        plan = ops.LMPlan(M, idx=idx, coeff=torch.as_tensor(rng.uniform(0.5, 2.0, K_in)))
        Ax = ops.lm_apply(x, plan, dim=1)
        yv = lc.rand(rng, (O, R, I), Ax.is_complex()).to(DEV)
        AHy, = torch.autograd.grad(Ax, x, yv)
        assert AHy.shape == x.shape and AHy.dtype == x.dtype
        lhs = torch.vdot(yv.reshape(-1), Ax.detach().reshape(-1))
        rhs = torch.vdot(AHy.reshape(-1), x.detach().reshape(-1))
        rel = float((lhs - rhs).abs() / lhs.abs())
        print('RATIO adjoint %s xc %d mc %d: %.2e' % (shape, xc, mc, rel))
        assert rel < 1e-12


CASES_ND = [(dict(dim=-2), (1, 2, 5, 300), 40), (dict(dim=1), (3, 40, 130), 7), (dict(dim=-1), (2, 67, 6), 65),
            (dict(dim=0), (9,), 20), (dict(dim=2, idx=True, coeff=True), (2, 3, 7, 65), 33),
            (dict(dim=-1, idx=True, coeff=True), (67, 8), 65), (dict(dim=-2, out_real=True), (2, 6, 129), 40)]


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('case', range(len(CASES_ND)))
def test_linear_model_forward_and_autograd_against_the_oracle(case, prec):
    """LinearModel.forward on tensors of 1 to 4 axes and its autograd gradient against the oracle's own autograd (float64 CPU),
    within the bound of the forward product and of the transposed product (plus the multiplicity of a repeated idx)"""
    from bayeslim_amd import linear_model as lm
    kw, shape, Ns = CASES_ND[case]
    dt = RDT[prec]
    rng = np.random.default_rng(100 + case)
    for xc, ac in ((False, False), (True, True), (True, False), (False, True)):
        if kw.get('out_real') and not (xc or ac):
            continue
        x = lc.rand(rng, shape, xc, dt)
        d = kw['dim'] % len(shape)
        L = shape[d]
        idx = torch.as_tensor([L - 1, 0, 0, 2, 2][:min(5, L)]) if kw.get('idx') else None
        K = L if idx is None else len(idx)
        A = lc.rand(rng, (Ns, K), ac, dt)
        cvec = torch.as_tensor(rng.uniform(0.5, 2.0, L)).to(dt) if kw.get('coeff') else None
        coeff = None if cvec is None else (cvec if d == len(shape) - 1 else cvec.reshape([-1 if a == d else 1 for a in range(len(shape))]))
        LM = lm.LinearModel('custom', A=A.to(DEV), dim=kw['dim'], idx=None if idx is None else idx.to(DEV),
                            coeff=None if coeff is None else coeff.to(DEV), out_real=bool(kw.get('out_real')))
        xg = x.to(DEV).requires_grad_(True)
        y = LM(xg)
        # oracle with autograd
        xo = lc._wide(x).requires_grad_(True)
        O, I = int(np.prod(shape[:d], dtype=np.int64)), int(np.prod(shape[d + 1:], dtype=np.int64))
        pre = None if cvec is None else (cvec if idx is None else cvec[idx])
        y64 = lc.oracle(xo.reshape(O, L, I), A, idx=idx, pre=pre, out_real=bool(kw.get('out_real')))
        B = lc.bound(x.reshape(O, L, I), A, dt, idx=idx, pre=pre)
        assert y.shape == shape[:d] + (Ns,) + shape[d + 1:] and y.is_complex() == y64.is_complex()
        rf = lc.ratio(y.reshape(O, Ns, I), y64.detach(), B)
        c = lc.rand(rng, tuple(y64.shape), y64.is_complex(), dt)
        g64, = torch.autograd.grad(y64, xo, lc._wide(c))
        gx, = torch.autograd.grad(y, xg, c.reshape(y.shape).to(DEV))
        assert gx.shape == x.shape and gx.dtype == x.dtype
        # bound of the transposed product, scattered: sum the compact bound over the entries that share an input
        mult = 1 if idx is None else int(torch.bincount(idx).max())
        Bc = lc.bound(c, A.conj().T.resolve_conj(), dt, post=pre, extra=mult - 1)
        if idx is not None:
            Bc = torch.zeros(O, L, I, dtype=torch.float64).index_add_(1, idx, Bc)
        rb = lc.ratio(gx.reshape(O, L, I), g64.reshape(O, L, I), Bc)
        print('RATIO LinearModel %s %s %s xc %d ac %d: fwd %.3f grad %.3f' % (kw, shape, prec, xc, ac, rf, rb))
        assert rf <= 1.0 and rb <= 1.0
    with pytest.raises(ValueError, match='requires grad'):
        lm.LinearModel('custom', A=torch.zeros(3, shape[d], device=DEV, requires_grad=True), dim=kw['dim'])(xg)


def test_non_contiguous_input_and_bitwise_repeatability():
    from bayeslim_amd import linear_model as lm
    rng = np.random.default_rng(11)
    for shape, dim, Ns in (((2, 7, 130), 1, 70), ((2, 40, 65), 1, 9), ((70, 6), 1, 65)):
        x = lc.rand(rng, shape, True, torch.float32).to(DEV)
        LM = lm.LinearModel('custom', A=lc.rand(rng, (Ns, shape[dim]), True, torch.float32).to(DEV), dim=dim)
        y = LM(x)
        xp = x.movedim(dim, 0).contiguous().movedim(0, dim)                     # the same values, permuted strides
        assert not xp.is_contiguous() or len(shape) == 1
        assert torch.equal(LM(xp), y)
        xg = x.clone().requires_grad_(True)
        g1, = torch.autograd.grad(LM(xg), xg, y)
        g2, = torch.autograd.grad(LM(xg), xg, y)
        assert torch.equal(LM(x), y) and torch.equal(g1, g2)


def _to_prec(t, prec):
    if t is None or not (t.is_floating_point() or t.is_complex()):
        return t
    return t.to((torch.complex64 if t.is_complex() else torch.float32) if prec == 'f32' else t.dtype)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_forward_and_multilm_fixtures_through_the_modules(prec):
    """every LinearModel.forward fixture and the MultiLM fixture of lm.npz on the GPU: float64 to 1e-10 of the output maximum,
    float32 within the bound (against the oracle on the rounded operands; the oracle meets the fixtures in test_lm_host.py)"""
    from bayeslim_amd import linear_model as lm
    g = lc.golden()
    for i, c in enumerate(lc.FWD_CASES):
        x, A, coeff, idx, d = lc.fwd_setup(g, c)
        x, A, coeff = (_to_prec(t, prec) for t in (x, A, coeff))
        dv = lambda t: None if t is None else t.to(DEV)
        y = lc.fwd_model(lm, dv(A), dv(coeff), dv(idx), c, c['dim'])(dv(x))
        ref = g['fwd_%d' % i]
        assert y.shape == ref.shape and y.is_complex() == ref.is_complex(), c
        if prec == 'f64':
            assert y.dtype == ref.dtype, c
            err = float((y.cpu() - ref).abs().max() / ref.abs().max())
            print('RATIO fixture fwd_%d f64: %.2e' % (i, err))
            assert err <= 1e-10, c
        elif not c.get('diag'):
            xm = x if coeff is None else x * coeff                  # the bound takes the product as the kernel's input ...
            fused = coeff is not None and c.get('coeff') == 'vec'
            O, I = int(np.prod(x.shape[:d], dtype=np.int64)), int(np.prod(x.shape[d + 1:], dtype=np.int64))
            y64 = lc.fwd_oracle(x, A, coeff, idx, d, dict(c, out_dtype=None, out_reshape=None))
            B = lc.bound(xm.reshape(O, x.shape[d], I), A, torch.float32, idx=idx, extra=0 if fused else 1)    # ... one rounding more
            r = lc.ratio(y.reshape(O, -1, I), y64.reshape(O, -1, I), B)
            print('RATIO fixture fwd_%d f32: %.3f' % (i, r))
            assert r <= 1.0, c
    if prec == 'f64':
        M = lm.MultiLM([lm.LinearModel('custom', A=g['fwd_Ar_3'].to(DEV), dim=1), lm.LinearModel('custom', A=g['multi_A2'].to(DEV), dim=-1)])
        y = M(g['fwd_xr'].to(DEV))
        err = float((y.cpu() - g['multi_out']).abs().max() / g['multi_out'].abs().max())
        print('RATIO fixture multi f64: %.2e' % err)
        assert y.shape == g['multi_out'].shape and err <= 1e-10


def test_least_squares_fixtures_in_float64(f64):
    from bayeslim_amd import linear_model as lm
    g = lc.golden()
    for i, c in enumerate(lc.LS_CASES):
        A, y, Ninv, kw = lc.ls_setup(g, c)
        L = lm.LinearModel('custom', A=A.to(DEV), dim=1)
        xh = L.least_squares(y.to(DEV), Ninv=None if Ninv is None else Ninv.to(DEV), **kw)
        ref = g['ls_%d' % i]
        assert xh.shape == ref.shape and xh.dtype == ref.dtype, c
        err = float((xh.cpu() - ref).abs().max() / ref.abs().max())
        print('RATIO fixture ls_%d f64: %.2e' % (i, err))
        assert err <= 1e-10, c
    # cached D, and the out_shape round trip
    L = lm.LinearModel('custom', A=g['ls_Ar'].to(DEV), dim=1, out_reshape=(2, lc.NS * 5), out_shape=(2, lc.NS, 5))
    y = L(g['ls_rt_x'].to(DEV))
    assert float((y.cpu() - g['ls_rt_y']).abs().max()) <= 1e-10 * float(g['ls_rt_y'].abs().max())
    xh = L.least_squares(y, cache_D=True)
    assert L._D is not None and L._D.shape == (3, 3)
    assert float((xh.cpu() - g['ls_rt_x']).abs().max()) <= 1e-10 * float(g['ls_rt_x'].abs().max())
    assert torch.equal(L.least_squares(y), xh)                              # through the cached D


def test_least_squares_in_float32_within_the_propagated_bound():
    """xhat = D A^H (Ninv y) in float32 against its float64 evaluation on the same rounded A, y, Ninv and the D the call
    returned; margin |D| Bz + gamma_{K+1} |D| |z64| (lm_common.ls_margin).  The returned float32 D itself against the float64
    inverse of the float64 normal matrix of the same rounded A and Ninv (lm_common.d_margin), and mode='lstsq' against the
    float64 solution of the same rounded problem (lm_common.lstsq_margin)"""
    from bayeslim_amd import linalg
    g = lc.golden()
    dt = torch.float32
    for i, c in enumerate(lc.LS_CASES):
        A, y, Ninv, kw = lc.ls_setup(g, c)
        A, y, Ninv = (_to_prec(t, 'f32') for t in (A, y, Ninv))
        xh, D = linalg.least_squares(A.to(DEV), y.to(DEV), dim=1, Ninv=None if Ninv is None else Ninv.to(DEV), **kw)
        if kw.get('mode') == 'lstsq':
            sw = None if Ninv is None else lc._wide(Ninv).sqrt()
            Aw = lc._wide(A) if sw is None else lc._wide(A) * sw[:, None]
            yw = lc._wide(y) if sw is None else lc._wide(y) * sw[None, :, None]
            Y = yw.movedim(1, 0).reshape(lc.NS, -1)
            X64 = torch.linalg.lstsq(Aw, Y).solution
            err = (lc._wide(xh).movedim(1, 0).reshape(3, -1) - X64).norm(dim=0)
            r = float((err / lc.lstsq_margin(Aw, X64, Y - Aw @ X64, dt)).max())
            print('RATIO least_squares ls_%d f32 (lstsq): %.3f' % (i, r))
            assert D is None and xh.dtype == torch.float32 and r <= 1.0, c
            continue
        if kw['norm'] in ('inv', 'pinv', 'chol'):
            A64 = lc._wide(A)
            Dinv = A64.conj().T @ (A64 if Ninv is None else lc._wide(Ninv)[:, None] * A64)
            D64 = torch.linalg.inv((Dinv.real if Dinv.is_complex() else Dinv) + kw.get('eps', 0) * torch.eye(3, dtype=torch.float64))
            rd = float(torch.linalg.matrix_norm(lc._wide(D) - D64, 2)) / lc.d_margin(A, Ninv, D64, dt)
            print('RATIO least_squares ls_%d f32 D: %.3f' % (i, rd))
            assert D.dtype == torch.float32 and rd <= 1.0, c
        w = lc._wide(y) if Ninv is None else lc._wide(y) * lc._wide(Ninv[None, :, None] if Ninv.ndim == 1 else Ninv)
        AH = A.conj().T.resolve_conj()
        z64 = lc.oracle(w, AH)
        Bz = lc.bound(w, AH, dt, extra=0 if Ninv is None else 1)
        D = lc._wide(D)
        if kw['norm'] in ('inv', 'pinv', 'chol'):
            x64, margin = lc.oracle(z64, D), lc.ls_margin(D, Bz, z64, 1, dt)
        elif kw['norm'] == 'diag':
            Dd = D[None, :, None] if D.ndim == 1 else D
            x64, margin = Dd * z64, Dd.abs() * (Bz + lc.gamma(1, dt) * z64.abs())
        else:
            x64, margin = z64, Bz
        r = lc.ratio(xh, x64, margin)
        print('RATIO least_squares ls_%d f32: %.3f' % (i, r))
        assert xh.dtype == (torch.complex64 if c.get('ac') else torch.float32) and r <= 1.0, c


def test_pickle_deepcopy_and_push_keep_the_bits():
    from bayeslim_amd import linear_model as lm
    rng = np.random.default_rng(5)
    x = lc.rand(rng, (2, 9, 130), True, torch.float32).to(DEV)
    A = lc.rand(rng, (40, 5), True, torch.float32)
    LM = lm.LinearModel('custom', A=A.to(DEV), dim=1, idx=torch.as_tensor([8, 0, 0, 3, 5], device=DEV),
                        coeff=torch.as_tensor(rng.uniform(0.5, 2, (1, 9, 1)), dtype=torch.float32, device=DEV), out_real=True)
    xg = x.clone().requires_grad_(True)
    y0 = LM(xg)
    g0, = torch.autograd.grad(y0, xg, torch.ones_like(y0))
    assert '_plans' in LM.__dict__ and y0.dtype == torch.float32

    def same(M):
        xg = x.clone().requires_grad_(True)
        y = M(xg)
        g, = torch.autograd.grad(y, xg, torch.ones_like(y))
        return torch.equal(y, y0) and torch.equal(g, g0)

    P, C = pickle.loads(pickle.dumps(LM)), copy.deepcopy(LM)
    assert '_plans' not in P.__dict__ and '_plans' not in C.__dict__
    assert same(P) and same(C)
    LM.push(torch.float64)
    assert LM.A.dtype == torch.complex128 and LM.coeff.dtype == torch.float64 and '_plans' not in LM.__dict__
    y64 = LM(x.to(torch.complex128))
    assert y64.dtype == torch.float64 and float((y64 - y0).abs().max()) < 1e-4 * float(y0.abs().max())
    LM.push(torch.float32)
    assert LM.A.dtype == torch.complex64 and same(LM)
    LM.push('cpu')
    assert LM.A.device.type == 'cpu' and LM.idx.device.type == 'cpu' and LM.device == 'cpu'
    LM.push(DEV)
    assert LM.A.is_cuda and same(LM)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_rime_lm_mini_against_the_reference(prec):
    """the drop-in RIME with bayeslim_amd.linear_model.LinearModel in the sky and the beam response (freq_mode='linear')
    against the reference's visibilities and gradients: float64 1e-10, float32 1e-5 (visibilities) and 1e-4 (gradients) of max"""
    from bayeslim_amd import utils, telescope_model, beam_model, sky_model, rime_model, linear_model as lm
    old = torch.get_default_dtype()
    torch.set_default_dtype(RDT[prec])
    try:
        g = {k: v.numpy() for k, v in lc.golden(lc.MINI).items()}
        rdt, cdt = RDT[prec], (torch.complex128 if prec == 'f64' else torch.complex64)
        T = lambda a, dt=None: torch.as_tensor(np.asarray(a)).to(dt or rdt).to(DEV)
        freqs = T(g['freqs'])
        antpos = utils.AntposDict(g['ants'].tolist(), torch.as_tensor(g['antvecs'], dtype=torch.float64))
        arr = telescope_model.ArrayModel(antpos, freqs=freqs, cache_s=True, redtol=1.0, device=DEV)
        tel = telescope_model.TelescopeModel((21.42827, -30.72148))
        fx = torch.as_tensor(g['freqs'], dtype=torch.float64)       # the basis is built in float64 and rounded once
        sky_LM = lm.LinearModel('poly', dim=-2, x=fx, Ndeg=3, basis='legendre', device=DEV)
        beam_LM = lm.LinearModel('poly', dim=-2, x=fx, Ndeg=2, basis='direct', device=DEV)
        tolA = 1e-12 if prec == 'f64' else 1e-6
        assert float((sky_LM.A.cpu().double() - g['sky_A']).abs().max()) <= tolA and sky_LM.A.is_cuda and sky_LM.A.dtype == rdt
        assert float((beam_LM.A.cpu().double() - g['beam_A']).abs().max()) <= tolA
        Rs = sky_model.PixelSkyResponse(freqs, freq_mode='linear', freq_LM=sky_LM, device=DEV)
        sky = sky_model.PixelSky(T(g['sky_params']), T(np.stack([g['ra'], g['dec']]), torch.float64), float(g['px_area']), R=Rs,
                                 parameter=True, name='lmsky')
        R = beam_model.PixelResponse(freqs, 'rect', interp_mode='linear', theta_grid=T(g['theta_grid'], torch.float64),
                                     phi_grid=T(g['phi_grid'], torch.float64), freq_mode='linear', freq_LM=beam_LM, powerbeam=True,
                                     realbeam=True, device=DEV)
        beam = beam_model.PixelBeam(T(g['beam_params']), freqs, R=R, pol='e', powerbeam=True, fov=180, parameter=True)
        sim_bls = [tuple(b) for b in g['sim_bls'].tolist()]
        rime = rime_model.RIME(sky, tel, beam, arr, sim_bls, g['times'], freqs)
        for t, za in zip(g['times'], g['zenaz']):
            tel.conv_cache[('lmsky', 192, float(t))] = torch.as_tensor(za, dtype=torch.float64)
        vis = rime().data
        assert vis.shape == (1, 1, 21, 2, 6) and vis.dtype == cdt
        rel = lambda a, b: float(np.abs(a.detach().cpu().numpy() - b).max() / np.abs(b).max())
        tv, tg = (1e-10, 1e-10) if prec == 'f64' else (1e-5, 1e-4)
        ev = rel(vis, g['vis'])
        loss = (vis * T(g['gvis'], cdt).conj()).real.sum()
        gs, gb = torch.autograd.grad(loss, [sky.params, beam.params])
        es, eb = rel(gs, g['g_sky_params']), rel(gb, g['g_beam_params'])
        print('RATIO rime_lm_mini %s: vis %.2e grad sky %.2e grad beam %.2e' % (prec, ev, es, eb))
        assert gs.shape == (1, 1, 3, 192) and gb.shape == tuple(g['beam_params'].shape)
        assert ev < tv and es < tg and eb < tg
    finally:
        torch.set_default_dtype(old)


def test_profile_tuples():
    """ops.PROFILE receives one ('lm_kernel', start, end, O R I K) per launch: the forward, then the adjoint of the backward"""
    from bayeslim_amd import ops
    rng = np.random.default_rng(6)
    A = torch.as_tensor(rng.normal(size=(5, 3))).float()
    x = torch.as_tensor(rng.normal(size=(3, 4))).float().to(DEV).requires_grad_(True)
    plan = ops.LMPlan(A)
    O, K, R, I = 1, 3, 5, 4
    prof = []
    ops.PROFILE = prof
    try:
        y = ops.lm_apply(x, plan, dim=0)
        assert y.shape == (R, I) and len(prof) == 1
        y.sum().backward()
    finally:
        ops.PROFILE = None
    torch.cuda.synchronize()
    assert len(prof) == 2 and all(len(k) == 4 and k[0] == 'lm_kernel' and k[3] == O * R * I * K for k in prof), prof
    assert all(k[1].elapsed_time(k[2]) >= 0 for k in prof)
    ops.lm_apply(x.detach(), plan, dim=0)
    assert len(prof) == 2                                      # nothing is recorded once PROFILE is None again
