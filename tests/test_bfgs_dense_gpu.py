"""
GPU checks of the dense BFGS kernels (csrc/bfgs.hip) and of bayeslim_amd/bfgs.py on them: rime_bfgs_matvec and rime_bfgs_rank2
against the float64 oracle of tests/bfgs_dense_common.py within its derived bounds, at the smallest shapes at which each
mechanism can break (a lone element, less than a 16-byte group, a ragged tail, a row that is not 16-byte aligned, exactly one
column chunk of float64, more than one chunk of either precision and more than one row group and tile), in a padded view and
one element off alignment; then BFGS trajectories, the factored form, implicit_to_dense and lbfgs_approx_cov against the
reference's record.
"""
import numpy as np
import pytest
import torch

import bfgs_dense_common as dc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = (torch.float32, torch.float64)
NS = (1, 2, 37, 97, 256, 300, 1030)


def matrix(rng, N, dtype, pad=0, offset=0, symmetric=False):
    """an (N, N) view with row stride N + pad whose first element sits `offset` elements into its storage"""
    A = rng.normal(size=(N, N))
    if symmetric:
        A = A + A.T
    buf = torch.full((N * (N + pad) + offset,), 7.0, dtype=dtype, device=DEV)
    H = buf[offset:].view(N, N + pad)[:, :N]
    H.copy_(torch.as_tensor(A).to(dtype))
    return H, buf


def vector(rng, shape, dtype, offset=0):
    n = int(np.prod(shape))
    buf = torch.empty(n + offset, dtype=dtype, device=DEV)
    buf[offset:] = torch.as_tensor(rng.normal(size=n)).to(dtype)
    return buf[offset:].view(shape)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_matvec_against_the_oracle_and_across_placements(dtype):
    from bayeslim_amd import bfgs
    rng = np.random.default_rng(21)
    worst = 0.0
    for N in NS:
        dense = bfgs._Dense(N, dtype, torch.device(DEV, torch.cuda.current_device()))
        H, _ = matrix(rng, N, dtype)
        for nrhs in (1, 2):
            x = vector(rng, (N,) if nrhs == 1 else (N, 2), dtype)
            r = dense.matvec(H, x)
            assert r.shape == x.shape and r.dtype == dtype
            q = dc.ratio(r.cpu().double() - dc.oracle_matvec(H, x), dc.matvec_bound(N, dtype, dc.oracle_matvec_abs(H, x)))
            worst = max(worst, q)
            assert q <= 1.0, ('matvec', N, nrhs, q)
            # the same data in a view of a wider matrix, one element off alignment, and both; a shifted x: identical bits
            for pad, off in ((3, 0), (0, 1), (3, 1)):
                H2, _ = matrix(rng, N, dtype, pad, off)
                H2.copy_(H)
                assert H2.stride(0) == N + pad and (off == 0 or H2.data_ptr() % 16 != 0)
                x2 = vector(rng, x.shape, dtype, offset=1)
                x2.copy_(x)
                assert torch.equal(dense.matvec(H2, x2), r), ('placement', N, nrhs, pad, off)
            if nrhs == 2:                                 # the two right-hand sides are the two single products, bit for bit
                assert torch.equal(r[:, 0], dense.matvec(H, x[:, 0].contiguous()))
                assert torch.equal(r[:, 1], dense.matvec(H, x[:, 1].contiguous()))
    assert dc.matvec_roundings(1030, torch.float32) == 26 and dc.matvec_roundings(2, dtype) == 2
    print('%s: worst matvec error / bound %.3f' % (dtype, worst))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_rank2_against_the_oracle_symmetry_padding_and_identity(dtype):
    from bayeslim_amd import bfgs
    rng = np.random.default_rng(22)
    worst = 0.0
    for N in NS:
        dense = bfgs._Dense(N, dtype, torch.device(DEV, torch.cuda.current_device()))
        x, z = vector(rng, (N,), dtype), vector(rng, (N,), dtype, offset=1)
        a, b = -0.37, 1.9
        outs = []
        for pad, off in ((0, 0), (3, 0), (0, 1), (3, 1)):
            H, buf = matrix(np.random.default_rng(100 + N), N, dtype, pad, off, symmetric=True)
            assert torch.equal(H, H.T)
            H_before, buf_before = H.clone(), buf.clone()
            assert dense.rank2(H, x, z, 0.0, 0.0) is H and torch.equal(H, H_before) and torch.equal(buf, buf_before)
            dense.rank2(H, x, z, a, b)
            q = dc.ratio(H.cpu().double() - dc.oracle_rank2(H_before, x, z, a, b),
                         dc.rank2_bound(dtype, dc.oracle_rank2_abs(H_before, x, z, a, b)))
            worst = max(worst, q)
            assert q <= 1.0, ('rank2', N, pad, off, q)
            assert torch.equal(H, H.T), ('symmetry', N, pad, off)
            # nothing outside the N columns of the N rows was written: the padding and the leading element keep their bits
            mask = torch.ones_like(buf, dtype=torch.bool)
            mask[off:].view(N, N + pad)[:, :N] = False
            assert torch.equal(buf[mask], buf_before[mask]), ('padding', N, pad, off)
            outs.append(H.clone())
        assert all(torch.equal(outs[0], o) for o in outs[1:]), ('placement', N)
    print('%s: worst rank2 error / bound %.3f' % (dtype, worst))


@pytest.mark.parametrize('kind,h0', dc.dense_cases())
def test_trajectory_against_the_reference(kind, h0):
    """bfgs.BFGS in float64 on the GPU on the reference's recorded trajectories: exit code, func_evals, n_iter and pair count
    equal, the floating-point record within FACTOR x the recorded discrepancy of the restatement; H stays bit-symmetric and the
    caller's H0 is not written"""
    from bayeslim_amd import bfgs
    g = dc.golden()
    icov, x0 = dc.dense_problem(g)
    H0 = dc.dense_H0(icov, h0).to(DEV)
    before = H0.clone()
    res, opt = dc.run_dense(bfgs.BFGS, icov, x0, H0, kind, device=DEV)
    e = dc.dense_discrepancy(res, g, kind, h0)
    print('dense trajectory %s %s on the GPU: %.3e' % (kind, h0, e))
    assert e <= dc.FACTOR * dc.DENSE_RESTATEMENT
    assert torch.equal(H0, before) and opt.H.is_cuda and opt.H.dtype == torch.float64 and torch.equal(opt.H, opt.H.T)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_step_launches_one_product_and_one_correction_per_iteration(dtype):
    """store_Hy off, through a launch counter in the seam: one rime_bfgs_matvec and one rime_bfgs_rank2 per completed iteration,
    plus the product of the very first direction; in float64 the direction kept for the next iteration is a fresh product H g
    within the restatement constant (float32: printed)"""
    from bayeslim_amd import bfgs
    g = dc.golden()
    icov, x0 = dc.dense_problem(g)
    calls = []

    class Counting(bfgs._Dense):
        def matvec(self, H, x):
            calls.append('matvec')
            return bfgs._Dense.matvec(self, H, x)

        def rank2(self, H, x, z, a, b):
            calls.append('rank2')
            return bfgs._Dense.rank2(self, H, x, z, a, b)

    class Opt(bfgs.BFGS):
        _dense_cls = Counting

    x = x0.to(dtype).to(DEV).requires_grad_(True)
    A = icov.to(dtype).to(DEV)
    opt = Opt((x,), max_iter=3)

    def closure():
        x.grad = None
        loss = 0.5 * (x @ (A @ x))
        loss.backward()
        return loss.detach()

    for step in range(2):
        opt.step(closure)
        assert opt.n_iter == 3 * (step + 1) and opt._exit == 0
        assert calls.count('matvec') == opt.n_iter + 1 and calls.count('rank2') == opt.n_iter, calls
    assert opt.H.dtype == dtype and torch.equal(opt.H, opt.H.T)
    e = dc.rel(opt._Hg[1].cpu().double(), dc.oracle_matvec(opt.H, opt._flat_grad))
    print('%s: kept direction against a fresh product %.3e' % (dtype, e))
    if dtype == torch.float64:
        assert e <= dc.FACTOR * dc.DENSE_RESTATEMENT


def _start_forms(icov):
    """(name, H0, L0) on the GPU: H0 = L0 L0^T in each form"""
    d = (1.0 / icov.diagonal()).to(DEV)
    from bayeslim_amd import hmat
    return (('none', None, None), ('diag', d, d.sqrt()), ('dense', torch.diag(d), torch.diag(d.sqrt())),
            ('DiagMat', hmat.DiagMat(d), hmat.DiagMat(d.sqrt())))


@pytest.mark.parametrize('kind', dc.FACTORED_KINDS)
def test_factored_inverse_hessian_against_the_reference(kind):
    from bayeslim_amd import bfgs
    g = dc.golden()
    N = dc.DENSE['N']
    a = dc.factored_args(g, kind)
    dev = lambda v: [t.to(DEV) for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v
    args = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else dev(v)) for k, v in a.items()}
    key = 'fact_%s_' % kind
    vec = g['fact_vec'].to(DEV)
    tol = dc.FACTOR * dc.FACTORED_RESTATEMENT
    icov, _ = dc.dense_problem(g)
    for name, H0, L0 in _start_forms(icov):
        F = bfgs.FactoredInvHessian(H0=H0, L0=L0, **args)
        assert len(F.u) == int(g[key + 'kept'][0]) and F.N == N and F.m == len(a['s'])
        assert dc.rel(torch.stack(F.u).cpu(), g[key + 'u']) <= tol and dc.rel(torch.stack(F.v).cpu(), g[key + 'v']) <= tol
        u, v = [t.cpu() for t in F.u], [t.cpu() for t in F.v]
        M_H = None if H0 is None else (H0.diagonal() if name == 'DiagMat' else H0).cpu()
        M_L = None if L0 is None else (L0.diagonal() if name == 'DiagMat' else L0).cpu()
        hv, lv, Hd, Ld = F.hvp(vec), F.lvp(vec), F.to_dense(True), F.to_dense(False)
        assert torch.equal(F(vec), lv) and Hd.is_cuda and Hd.shape == Ld.shape == (N, N)
        if name == 'none':                                # the reference's own record
            want = (g[key + 'hvp'], g[key + 'lvp'], dc.from_triu(g[key + 'H_triu'], N), g[key + 'L'])
        else:                                             # the compact form on the CPU, itself checked against the record
            want = (dc.host_shells(vec, M_H, u, v, True), dc.host_shells(vec, M_L, u, v, False),
                    dc.host_to_dense(M_H, u, v, True), dc.host_to_dense(M_L, u, v, False))
        e = max(dc.rel(x.cpu(), w) for x, w in zip((hv, lv, Hd, Ld), want))
        print('factored %s %s: %.3e' % (kind, name, e))
        assert e <= tol
        # hvp(v) = to_dense(True) v = L (L^T v), and the module functions give what the object gives
        assert dc.rel(hv.cpu(), Hd.cpu() @ vec.cpu()) <= tol and dc.rel(hv.cpu(), Ld.cpu() @ (Ld.cpu().T @ vec.cpu())) <= tol
        assert torch.equal(bfgs.factored_hvp(vec, H0, F.u, F.v), hv) and torch.equal(bfgs.factored_lvp(vec, L0, F.u, F.v), lv)
        two = torch.stack([vec, 2.0 * vec], dim=1)
        assert torch.equal(F.lvp(two)[:, 0], lv) and torch.equal(F.hvp(two)[:, 0], hv) and F.hvp(two).shape == (N, 2)
    if kind == 'rank2':
        Hfin = dc.from_triu(g['dense_%s_%s_H_triu' % dc.FACTORED_RUN], N)
        F = bfgs.FactoredInvHessian(**args)
        assert dc.rel(F.to_dense(True).cpu(), Hfin) <= dc.FACTOR * dc.FACTORED_VS_BFGS
    assert torch.equal(bfgs.factored_hvp(vec, None, [], []), vec)


@pytest.mark.parametrize('h0', dc.ITD_H0S)
def test_implicit_to_dense_against_the_reference(h0):
    from bayeslim_amd import bfgs, hmat
    g = dc.golden()
    s, y = [[t.to(DEV) for t in v] for v in dc.factored_lists(g)[:2]]
    H0 = dc.itd_H0(g, h0)
    H0 = None if H0 is None else H0.to(DEV)
    want = dc.from_triu(g['itd_%s_H_triu' % h0], dc.DENSE['N'])
    e = dc.rel(bfgs.implicit_to_dense(H0, s, y).cpu(), want)
    print('implicit_to_dense %s on the GPU: %.3e' % (h0, e))
    assert e <= dc.FACTOR * dc.DENSE_RESTATEMENT
    if h0 == 'diag':
        assert dc.rel(bfgs.implicit_to_dense(hmat.DiagMat(H0), s, y).cpu(), want) <= dc.FACTOR * dc.DENSE_RESTATEMENT


def test_lbfgs_approx_cov_on_a_two_group_quadratic():
    from bayeslim_amd import bfgs, hmat
    prob, sizes = dc.quadratic_logprob(DEV)
    names = dict(prob._main_names)
    D = bfgs.lbfgs_approx_cov(prob, Nsteps=3, max_iter=2)
    assert isinstance(D, hmat.DiagMat) and D.diagonal().shape == (sum(sizes),) and D.diagonal().is_cuda
    assert dict(prob._main_names) == names and prob.main_params.numel() == sum(sizes)
    want = dc.hdiag_by_hand(bfgs.LBFGS, DEV, Nsteps=3, max_iter=2)
    assert torch.equal(D.diagonal(), want) and bool((want > 0).all()) and len(set(want.tolist())) == 2
