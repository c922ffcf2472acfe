"""
CPU-side checks of the linear-model layer (bayeslim_amd/linear_model.py, linalg.py, utils.prep_xarr, ops.LMPlan,
rime_lm_apply): the bases, prep_xarr and gen_fourier_A against the reference's recorded results (tests/golden/lm.npz), the
float64 oracle of tests/lm_common.py (what the GPU tests compare with) against every forward and least_squares fixture, the
A^H tables of the plan, argument validation without a GPU, and the no-scratch property of the built kernels.
"""
import copy
import ctypes
import pickle
import warnings

import numpy as np
import pytest
import torch

import lm_common as lc
import kernel_asm


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape and a.is_complex() == b.is_complex(), (a.shape, b.shape, a.dtype, b.dtype)
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize('basis', lc.BASES)
def test_gen_poly_A_against_the_reference(f64, basis):
    from bayeslim_amd import linear_model as lm
    g = lc.golden()
    for Ndeg in lc.NDEGS:
        for xn in lc.XNAMES:
            for w in (0, 1):
                A = lm.gen_poly_A(g['x_' + xn], Ndeg, basis=basis, whiten=bool(w))
                assert A.dtype == torch.float64 and A.shape == (12, Ndeg)
                assert close(A, g['poly_%s_%d_%s_%d' % (basis, Ndeg, xn, w)]), (basis, Ndeg, xn, w)
    with pytest.raises(NameError):
        lm.gen_poly_A(g['x_uni'], 3, basis='hermite')


def test_gen_poly_A_options_and_prep_xarr(f64):
    from bayeslim_amd import linear_model as lm, utils
    g = lc.golden()
    for name, kw in lc.POLY_OPTS.items():
        assert close(lm.gen_poly_A(g['x_nonuni'], 4, basis='legendre', **kw), g['poly_opt_%s' % name]), name
        assert close(lm.gen_linear_A('poly', x=g['x_nonuni'], Ndeg=4, basis='legendre', **kw), g['poly_opt_%s' % name]), name
    Q = lm.gen_poly_A(g['x_nonuni'], 4, basis='chebyshevt', qr=True)
    assert float((Q.T @ Q - torch.eye(4)).abs().max()) < 1e-13
    for name, kw in lc.PREP_OPTS.items():
        x, x0, dx = utils.prep_xarr(g['x_nonuni'], **kw)
        assert close(x, g['prep_%s_x' % name]), name
        want = g['prep_%s_x0dx' % name]
        for v, w in zip((x0, dx), want):
            assert (v is None and bool(torch.isnan(w))) or abs(float(v) - float(w)) <= 1e-12 * abs(float(w)), name
    xw, x0, dx = utils.whiten_xarr(g['x_uni'])
    assert abs(float(xw[-1]) - (1 - 1.0 / 12)) < 1e-12 and abs(float(xw[0]) + (1 - 1.0 / 12)) < 1e-12
    assert lm.gen_poly_A(g['x_uni'], 3).dtype == torch.float64
    torch.set_default_dtype(torch.float32)
    assert lm.gen_poly_A(g['x_uni'], 3).dtype == torch.float32


def test_gen_fourier_A_against_the_reference(f64):
    from bayeslim_amd import linear_model as lm
    g = lc.golden()
    for Ndeg, norm in lc.FOURIER:
        A, f = lm.gen_fourier_A(g['x_uni'], Ndeg=Ndeg, fft_norm=norm)
        assert A.is_complex() and A.shape == (12, 12 if Ndeg is None else Ndeg)
        assert close(A, g['four_%s_%s_A' % (Ndeg, norm)]) and close(f, g['four_%s_%s_freqs' % (Ndeg, norm)])
    # the default dtype of gen_linear_A is REAL, as in the reference: the imaginary part is dropped (make_golden_lm.py)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        A = lm.gen_linear_A('fourier', x=g['x_uni'])
        L = lm.LinearModel('fourier', x=g['x_uni'], Ndeg=5)
    assert not A.is_complex() and close(A, g['four_default'])
    assert not L.A.is_complex() and close(L.freqs, g['four_5_ortho_freqs'])
    Ac = lm.gen_linear_A('fourier', x=g['x_uni'], Ndeg=5, dtype=torch.complex128)
    assert Ac.is_complex() and close(Ac, g['four_complex']) and close(Ac, g['four_5_ortho_A'])
    with pytest.raises(NameError):
        lm.gen_linear_A('wavelet', x=g['x_uni'])


@pytest.mark.parametrize('case', range(len(lc.FWD_CASES)))
def test_oracle_against_the_forward_fixtures(f64, case):
    """the float64 oracle of lm_common on the reference's LinearModel.forward outputs; diag=True runs the module itself
    (an elementwise torch product that needs no GPU)"""
    from bayeslim_amd import linear_model as lm
    g = lc.golden()
    c = lc.FWD_CASES[case]
    x, A, coeff, idx, d = lc.fwd_setup(g, c)
    ref = g['fwd_%d' % case]
    if c.get('diag'):
        y = lc.fwd_model(lm, A, coeff, idx, c, c['dim'])(x)
        assert close(lc.fwd_model(lm, A, coeff, idx, c, c['dim'] - x.ndim)(x), ref)        # a negative dim as well
    else:
        y = lc.fwd_oracle(x, A, coeff, idx, d, c)
    assert close(y, ref), c


def test_oracle_against_the_multilm_and_least_squares_fixtures(f64):
    g = lc.golden()
    y = lc.fwd_oracle(g['fwd_xr'], g['fwd_Ar_3'], None, None, 1, {})
    assert close(lc.fwd_oracle(y, g['multi_A2'], None, None, 3, {}), g['multi_out'])
    for i, c in enumerate(lc.LS_CASES):
        A, y, Ninv, kw = lc.ls_setup(g, c)
        xhat = ls_oracle(A, y, Ninv, **kw)
        assert close(xhat, g['ls_%d' % i], 1e-12 if kw.get('mode') != 'lstsq' else 1e-10), c


def ls_oracle(A, y, Ninv=None, mode='matrix', norm='inv', pinv=True, eps=0, rcond=1e-15, hermitian=True, D=None):
    """xhat = D A^H (Ninv y) along axis 1 of y (2, NS, 5) in float64 through oracle(); the normal equations for 'lstsq'"""
    w = y if Ninv is None else y * (Ninv[None, :, None] if Ninv.ndim == 1 else Ninv)
    z = lc.oracle(w, A.conj().T)
    if mode == 'lstsq':
        norm, eps, pinv = 'inv', 0, False
    if norm in ('inv', 'pinv', 'chol'):
        if D is None:
            Dinv = A.conj().T @ (A if Ninv is None else Ninv[:, None] * A)
            Dinv = (Dinv.real if Dinv.is_complex() else Dinv) + eps * torch.eye(A.shape[1])
            D = torch.linalg.pinv(Dinv, rcond=rcond, hermitian=hermitian) if (norm == 'pinv' or (pinv and norm == 'inv')) else torch.linalg.inv(Dinv)
        return lc.oracle(z, D)
    if norm == 'diag':
        A2 = A.abs() ** 2
        if Ninv is None:
            return z / A2.sum(0)[None, :, None]
        if Ninv.ndim == 1:
            return z / (Ninv[:, None] * A2).sum(0)[None, :, None]
        return z / lc.oracle(Ninv, A2.T)
    return z


def test_plan_tables_against_the_conjugate_transpose():
    from bayeslim_amd import ops
    rng = np.random.default_rng(3)
    for cplx in (False, True):
        A = lc.rand(rng, (7, 3), cplx)
        plan = ops.LMPlan(A, idx=[2, 0, 0], coeff=torch.as_tensor([0.5, 9.0, 2.0, 7.0]))
        assert (plan.R, plan.K, plan.K_in, plan.cplx) == (7, 3, 4, cplx)
        for dt in (torch.float64, torch.float32):
            Ad = A.to(ops._lib_cdtype(dt) if cplx else dt)
            for layout in ('rk', 'kr'):
                buf, rs, ks, R, K, mc = plan.table('bwd', False, layout, dt, 'cpu')
                assert (R, K, mc) == (3, 7, cplx) and buf.is_contiguous() and (rs, ks) == ((7, 1) if layout == 'rk' else (1, 3))
                assert torch.equal(plan.matrix('bwd', False, layout, dt, 'cpu'), Ad.conj().T.resolve_conj())
                assert torch.equal(plan.matrix('fwd', False, layout, dt, 'cpu'), Ad)
                assert torch.equal(plan.matrix('bwd', True, layout, dt, 'cpu'), (Ad.real if cplx else Ad).T)
                flat = buf.reshape(-1) if not mc else buf.reshape(-1)
                assert flat[2 * rs + 5 * ks] == Ad.conj().T[2, 5]
            assert torch.equal(plan.scale(dt, 'cpu'), torch.as_tensor([2.0, 0.5, 0.5], dtype=dt))
        assert plan.gather('cpu').dtype == torch.int32 and plan.gather('cpu').tolist() == [2, 0, 0]
        for Q in (pickle.loads(pickle.dumps(plan)), copy.deepcopy(plan)):
            assert '_tabs' not in Q.__dict__ and torch.equal(Q.A, plan.A) and Q.idx.tolist() == [2, 0, 0]
            assert torch.equal(Q.table('bwd', False, 'kr', torch.float32, 'cpu')[0], plan.table('bwd', False, 'kr', torch.float32, 'cpu')[0])
    assert ops.lm_layout(256, 8, 100) == 'rk' and ops.lm_layout(8, 256, 100) == 'kr' and ops.lm_layout(256, 8, 1) == 'kr'
    assert ops.lm_layout(5, 32, 2) == 'rk' and ops.lm_layout(5, 33, 2) == 'kr'
    with pytest.raises(ValueError):
        ops.LMPlan(torch.zeros(3, 2, requires_grad=True))
    with pytest.raises(ValueError):
        ops.LMPlan(torch.zeros(2, 3, 4))
    with pytest.raises(IndexError):
        ops.LMPlan(torch.zeros(3, 2), idx=[0, 4], coeff=torch.ones(4))
    with pytest.raises(TypeError):
        ops.LMPlan(torch.zeros(3, 2), coeff=torch.ones(2, dtype=torch.complex64))


def test_entry_point_rejects_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)      # non-null dummy; never dereferenced on a rejected call

    def call(dtype=0, xc=0, mc=0, oreal=0, x=one, M=one, rs=4, ks=1, idx=None, pre=None, post=None, O=2, K=4, K_in=4, R=3, I=5,
             y=one):
        return lib.rime_lm_apply(dtype, xc, mc, oreal, x, M, rs, ks, idx, pre, post, O, K, K_in, R, I, y, None)

    assert call(dtype=2) == -1 and call(dtype=-1) == -1                         # unknown dtype
    assert call(K=0, K_in=0) == -1 and call(K=-1, K_in=-1) == -1 and call(R=0) == -1 and call(O=0) == -1 and call(I=0) == -1
    assert call(O=-3) == -1 and call(I=-1) == -1 and call(R=-2) == -1
    assert call(x=None) == -1 and call(M=None) == -1 and call(y=None) == -1     # null data pointers
    assert call(oreal=1) == -1 and call(oreal=1, mc=1) == -1                    # out_real with a real x
    assert call(idx=one, K_in=0) == -1 and call(idx=one, K_in=-2) == -1         # a gather into an empty axis
    assert call(K_in=5) == -1                                                   # no gather: K_in is K
    assert call(xc=2) == -1 and call(mc=-1) == -1 and call(oreal=3, xc=1) == -1
    assert call(rs=0) == -1 and call(ks=-1) == -1
    assert call(O=2 ** 62, I=4) == -1 and call(O=2 ** 40, I=2 ** 20, R=2 ** 10) == -1      # offsets beyond 62 bits
    assert call(O=2 ** 40, I=2 ** 20, K=2 ** 10, K_in=2 ** 10, rs=2 ** 10) == -1


def test_lm_apply_refuses_cpu_tensors_and_a_batched_A():
    from bayeslim_amd import ops, linear_model as lm, linalg, filt
    assert linalg.invert_matrix is filt.invert_matrix                       # one implementation
    plan = ops.LMPlan(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ops.lm_apply(torch.zeros(2, 3, 5), plan, dim=1)
    L = lm.LinearModel('custom', A=torch.zeros(4, 3), dim=1)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        L(torch.zeros(2, 3, 5))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        L.least_squares(torch.zeros(2, 4, 5))
    with pytest.raises(NotImplementedError, match='batched A'):
        lm.LinearModel('custom', A=torch.zeros(2, 4, 3), dim=1)(torch.zeros(2, 3, 5))
    for kw in (dict(pretran=True), dict(preconj=True), dict(Ninv=torch.eye(4), Ndiag=False)):
        with pytest.raises(NotImplementedError):
            linalg.least_squares(torch.zeros(4, 3), torch.zeros(2, 4, 5), dim=1, **kw)
    with pytest.raises(NotImplementedError):
        linalg.least_squares(torch.zeros(2, 4, 3), torch.zeros(2, 4, 5), dim=1)
    # 'lstsq' needs no kernel
    A, y = torch.randn(6, 3, dtype=torch.float64), torch.randn(2, 6, 5, dtype=torch.float64)
    xh, D = linalg.least_squares(A, y, dim=1, mode='lstsq')
    assert D is None and float((xh - torch.einsum('kj,ajb->akb', torch.linalg.pinv(A), y)).abs().max()) < 1e-12
    Dm = linalg.invert_matrix(torch.diag(torch.tensor([2.0, 4.0])), inv='inv')
    assert torch.equal(Dm, torch.diag(torch.tensor([0.5, 0.25])))
    assert torch.equal(linalg.invert_matrix(torch.tensor([2.0, 4.0])), torch.tensor([0.5, 0.25]))
    assert torch.equal(linalg.invert_matrix(torch.tensor([[2.0, 1.0], [1.0, 4.0]]), inv='diag'), torch.diag(torch.tensor([0.5, 0.25])))


def test_linear_model_attributes_pickle_and_containers(f64):
    from bayeslim_amd import linear_model as lm
    g = lc.golden()
    L = lm.LinearModel('poly', dim=-2, x=g['x_uni'], Ndeg=4, basis='legendre', whiten=True, meta={'a': 1})
    assert L.A.shape == (12, 4) and L.linear_mode == 'poly' and L.dim == -2 and L.freqs is None and L.meta == {'a': 1}
    assert 'x0' in L.kwargs and 'dx' in L.kwargs and L.device == L.A.device and L._D is None and not L.diag
    assert close(L.A, g['poly_legendre_4_uni_1'])
    assert close(L.generate_A(g['x_uni']), L.A) and L.generate_A(g['x_nonuni'][:5]).shape == (5, 4)
    L.__dict__['_plans'] = {'k': None}
    for Q in (pickle.loads(pickle.dumps(L)), copy.deepcopy(L)):
        assert '_plans' not in Q.__dict__ and torch.equal(Q.A, L.A) and Q.kwargs.keys() == L.kwargs.keys()
    L.__dict__.pop('_plans')
    V = lm.LinearModel('custom', A=torch.arange(1.0, 4.0), dim=0)             # a 1-D A: one feature
    p1 = V._plan('fwd', V.A)
    assert V._plan('fwd', V.A) is p1 and (p1.R, p1.K) == (3, 1) and V._plan('ls', V.A) is not p1 and len(V._plans) == 2
    V.A.mul_(2.0)                                                             # an in-place edit is a new version: a new plan
    p2 = V._plan('fwd', V.A)
    assert p2 is not p1 and V._plan('fwd', V.A) is p2
    V.A = V.A.clone()                                                         # a replaced tensor as well
    assert V._plan('fwd', V.A) is not p2
    L.push(torch.float32)
    assert L.A.dtype == torch.float32 and '_plans' not in L.__dict__
    C = lm.LinearModel('custom', A=g['fwd_Ar_4'], x=torch.arange(6.0), dim=0)
    assert C.generate_A(np.array([0.5, 1.5])).shape == (2, 4)
    D = lm.LinearModel('custom', A=torch.diag(torch.tensor([1.0, 2.0, 3.0])), diag=True, dim=1)
    assert D.A.tolist() == [1.0, 2.0, 3.0] and D._A_ndim == 2
    M = lm.MultiLM([D, lm.LinearModel('custom', A=torch.diag(torch.tensor([2.0, 2.0])), diag=True, dim=0)])
    assert torch.equal(M(torch.ones(2, 3)), torch.tensor([[2.0, 4.0, 6.0]] * 2))
    DL = lm.DictLM({'p': D})
    assert torch.equal(DL('p', torch.ones(2, 3)), torch.tensor([[1.0, 2.0, 3.0]] * 2)) and DL.device == D.device
    DL.push(torch.float32)
    assert D.A.dtype == torch.float32


def test_lm_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/lm.hip: no kernel has a private segment"""
    _, kernels, sizes = kernel_asm.read('lm')
    # 2 precisions x 6 type combinations x (9 few-in + 9 few-out (register size, columns per lane) pairs + 1 last-axis)
    assert len(kernels) == 228 and all('lm_' in k for k in kernels), len(kernels)
    assert len(sizes) == 228 and max(sizes) == 0, sizes
