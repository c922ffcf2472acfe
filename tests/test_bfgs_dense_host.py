"""
CPU-side checks of the dense half of the optimiser layer (bayeslim_amd/bfgs.py: BFGS, factor_pairs, the compact shell
recurrences, implicit_to_dense; rime_bfgs_matvec, rime_bfgs_rank2): the restated step() on the float64 oracle of
tests/bfgs_dense_common.py against the reference's recorded trajectories (tests/golden/bfgs_dense.npz), the factored form
against its records, argument validation without a GPU, the refusals of the Python layer and the no-scratch property of the
built kernels.
"""
import ctypes
import math

import pytest
import torch

import bfgs_dense_common as dc
import kernel_asm


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


@pytest.mark.parametrize('kind,h0', dc.dense_cases())
def test_restated_step_reproduces_the_reference_trajectory(f64, kind, h0):
    """bfgs.BFGS.step on the float64 oracle (one product and one rank-two correction per iteration, no kernel): exit code,
    func_evals, n_iter and pair count equal, the floating-point record within FACTOR x DENSE_RESTATEMENT; the caller's H0 is
    not written, self.H is the parameters' dtype and stays symmetric bit for bit"""
    g = dc.golden()
    icov, x0 = dc.dense_problem(g)
    H0 = dc.dense_H0(icov, h0)
    before = H0.clone()
    res, opt = dc.run_dense(dc.host_bfgs(), icov, x0, H0, kind)
    e = dc.dense_discrepancy(res, g, kind, h0)
    print('dense trajectory %s %s: %.3e' % (kind, h0, e))
    assert e <= dc.FACTOR * dc.DENSE_RESTATEMENT
    assert torch.equal(H0, before) and opt.H.data_ptr() != H0.data_ptr()
    assert opt.H.dtype == torch.float64 and opt.H.shape == (dc.DENSE['N'],) * 2 and torch.equal(opt.H, opt.H.T)
    assert opt.n_iter == dc.DENSE['max_iter'] * dc.DENSE['steps']


def test_step_costs_one_product_and_one_correction_per_iteration(f64):
    """store_Hy off: the u / w identities leave one matvec and one rank2 per completed iteration, plus the product of the
    very first direction; a later step() starts from the cached product"""
    g = dc.golden()
    icov, x0 = dc.dense_problem(g)
    calls = []

    class Counting(dc.OracleDense):
        def matvec(self, H, x):
            calls.append('matvec')
            return dc.OracleDense.matvec(self, H, x)

        def rank2(self, H, x, z, a, b):
            calls.append('rank2')
            return dc.OracleDense.rank2(self, H, x, z, a, b)

    class Opt(dc.host_bfgs()):
        _dense_cls = Counting

    x = x0.clone().requires_grad_(True)
    opt = Opt((x,), max_iter=3)

    def closure():
        x.grad = None
        loss = 0.5 * (x @ (icov @ x))
        loss.backward()
        return loss.detach()

    for step in range(2):
        opt.step(closure)
        assert opt.n_iter == 3 * (step + 1) and opt._exit == 0
        assert calls.count('matvec') == opt.n_iter + 1 and calls.count('rank2') == opt.n_iter, calls
    # the direction kept for the next iteration is the product with the updated matrix
    assert dc.rel(opt._Hg[1], dc.oracle_matvec(opt.H, opt._flat_grad)) <= dc.FACTOR * dc.DENSE_RESTATEMENT


def test_update_hessian_refuses_a_pair_without_curvature(f64):
    x = torch.zeros(5, requires_grad=True)
    opt = dc.host_bfgs()((x,), H0=2.0)
    H = opt.H.clone()
    s = torch.arange(1.0, 6.0)
    assert opt.update_hessian(s, -s) is None and opt.update_hessian(s, torch.zeros(5)) is None
    assert torch.equal(opt.H, H) and opt._s is None and torch.equal(H, 2.0 * torch.eye(5))
    y = 0.5 * s
    rho, b = opt.update_hessian(s, y, alpha=0.25)
    assert opt._s is s and opt._y is y and opt._alpha == 0.25 and opt._rho == rho == 1.0 / float(s @ y)
    # the secant equation H y = s, and the reference's own expression of the update
    V = torch.eye(5) - rho * torch.outer(y, s)
    want = V.T @ H @ V + rho * torch.outer(s, s)
    assert dc.rel(opt.H, want) <= 1e-14 and dc.rel(opt.hvp(y), s) <= 1e-14
    z = torch.complex(s, y)
    assert torch.equal(opt.hvp(z), torch.complex(opt.hvp(s), opt.hvp(y)))


def test_factor_pairs_against_the_reference(f64):
    from bayeslim_amd import bfgs
    g = dc.golden()
    worst = 0.0
    for i, case in enumerate(dc.PAIR_CASES):
        s, y, gk, alpha, Hy = dc.pair_inputs(case)
        u, v, spd = bfgs.factor_pairs(s, y, gk, alpha, Hy, pos=case[2], rank2=case[1])
        assert int(bool(spd)) == int(g['pair_spd'][i])
        worst = max(worst, dc.rel(u, g['pair_%d_u' % i]), dc.rel(v, g['pair_%d_v' % i]))
    assert g['pair_spd'].tolist().count(0) >= 1
    with pytest.raises(ValueError, match='Hy_k'):
        bfgs.factor_pairs(s, y, gk, alpha, None, rank2=False)
    # the pairs of the recorded run
    for kind in dc.FACTORED_KINDS:
        a = dc.factored_args(g, kind)
        grads = [a['g_end'] - torch.stack(a['y'][k:]).sum(0) for k in range(len(a['s']))]
        us, vs = [], []
        for k in range(len(a['s'])):
            u, v, spd = bfgs.factor_pairs(a['s'][k], a['y'][k], grads[k], a['alpha'][k], a['Hy'][k], rank2=a['rank2'])
            if bool(spd):
                us.append(u)
                vs.append(v)
        assert len(us) == int(g['fact_%s_kept' % kind][0])
        worst = max(worst, dc.rel(torch.stack(us), g['fact_%s_u' % kind]), dc.rel(torch.stack(vs), g['fact_%s_v' % kind]))
    print('factor_pairs: %.3e' % worst)
    assert worst <= dc.FACTOR * dc.FACTORED_RESTATEMENT


@pytest.mark.parametrize('kind', dc.FACTORED_KINDS)
def test_compact_shells_reproduce_the_factored_products(f64, kind):
    """forward_shell / reverse_shell fed with numpy Gram matrices of the recorded u, v against the reference's hvp, lvp and
    to_dense; and a diagonal and a dense starting matrix against the shells applied one by one"""
    g = dc.golden()
    key = 'fact_%s_' % kind
    u, v, vec, N = list(g[key + 'u']), list(g[key + 'v']), g['fact_vec'], dc.DENSE['N']
    e = max(dc.rel(dc.host_shells(vec, None, u, v, True), g[key + 'hvp']),
            dc.rel(dc.host_shells(vec, None, u, v, False), g[key + 'lvp']),
            dc.rel(dc.host_to_dense(None, u, v, True), dc.from_triu(g[key + 'H_triu'], N)),
            dc.rel(dc.host_to_dense(None, u, v, False), g[key + 'L']))
    print('compact shells %s: %.3e' % (kind, e))
    assert e <= dc.FACTOR * dc.FACTORED_RESTATEMENT
    icov, _ = dc.dense_problem(g)
    for M in (1.0 / icov.diagonal(), torch.linalg.inv(icov)):
        for both in (False, True):
            x = vec.clone()
            if both:
                for u_k, v_k in zip(reversed(u), reversed(v)):
                    x = x + v_k * (u_k @ x)
            x = M * x if M.ndim == 1 else M @ x
            for u_k, v_k in zip(u, v):
                x = x + u_k * (v_k @ x)
            assert dc.rel(dc.host_shells(vec, M, u, v, both), x) <= dc.FACTOR * dc.FACTORED_RESTATEMENT


def test_factored_to_dense_equals_the_final_matrix_of_the_run(f64):
    """rank two: the product form is the BFGS matrix itself, so the replayed shells give the recorded final BFGS.H of the run"""
    g = dc.golden()
    N = dc.DENSE['N']
    Hfin = dc.from_triu(g['dense_%s_%s_H_triu' % dc.FACTORED_RUN], N)
    assert dc.rel(dc.from_triu(g['fact_rank2_H_triu'], N), Hfin) <= dc.FACTORED_VS_BFGS * (1 + 1e-12)
    e = dc.rel(dc.host_to_dense(None, list(g['fact_rank2_u']), list(g['fact_rank2_v']), True), Hfin)
    print('replayed shells against the final BFGS.H: %.3e' % e)
    assert e <= dc.FACTOR * dc.FACTORED_VS_BFGS


@pytest.mark.parametrize('h0', dc.ITD_H0S)
def test_implicit_to_dense_through_the_oracle(f64, h0, monkeypatch):
    from bayeslim_amd import bfgs
    monkeypatch.setattr(bfgs.BFGS, '_dense_cls', dc.OracleDense)
    g = dc.golden()
    s, y = dc.factored_lists(g)[:2]
    H0 = dc.itd_H0(g, h0)
    before = None if H0 is None else H0.clone()
    H = bfgs.implicit_to_dense(H0, s, y)
    e = dc.rel(H, dc.from_triu(g['itd_%s_H_triu' % h0], dc.DENSE['N']))
    print('implicit_to_dense %s: %.3e' % (h0, e))
    assert e <= dc.FACTOR * dc.DENSE_RESTATEMENT
    assert H0 is None or torch.equal(H0, before)


def test_entry_points_reject_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    H, x, z, r = (ctypes.c_void_p(1 << 40), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21), ctypes.c_void_p(1 << 22))
    nan, inf = math.nan, math.inf

    def mv(dtype=0, H=H, ld=100, N=100, x=x, nrhs=1, r=r):
        return lib.rime_bfgs_matvec(dtype, H, ld, N, x, nrhs, r, None)

    def r2(dtype=0, H=H, ld=100, N=100, x=x, z=z, a=1.0, b=1.0):
        return lib.rime_bfgs_rank2(dtype, H, ld, N, x, z, a, b, None)

    for f in (mv, r2):
        assert f(dtype=2) == -1 and f(dtype=-1) == -1                       # unknown dtype
        assert f(N=0) == -1 and f(N=-3) == -1 and f(N=1 << 31) == -1
        assert f(ld=99) == -1 and f(ld=0) == -1 and f(ld=-100) == -1       # ld < N
        assert f(H=None) == -1 and f(x=None) == -1
        assert f(x=H) == -1                                                 # a vector inside H
    assert mv(r=None) == -1 and mv(nrhs=0) == -1 and mv(nrhs=3) == -1 and mv(nrhs=-1) == -1
    assert mv(r=ctypes.c_void_p((1 << 40) + 4 * 100 * 50)) == -1            # the result inside H
    assert r2(z=None) == -1 and r2(z=ctypes.c_void_p((1 << 40) + 8)) == -1
    for bad in (nan, inf, -inf):
        assert r2(a=bad) == -1 and r2(b=bad) == -1


def test_python_layer_refusals(f64):
    from bayeslim_amd import bfgs
    x = torch.zeros(5, requires_grad=True)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        bfgs.BFGS((x,))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        bfgs.implicit_to_dense(None, [torch.ones(5)], [torch.ones(5)])
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        bfgs.factored_lvp(torch.ones(5), None, [torch.ones(5)], [torch.ones(5)])
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        bfgs.factored_hvp(torch.ones(5), torch.eye(5), [], [])
    with pytest.raises(NotImplementedError, match='complex parameters'):
        bfgs.BFGS((torch.zeros(5, dtype=torch.complex128, requires_grad=True),))
    with pytest.raises(NotImplementedError, match='complex parameters'):
        dc.host_bfgs()((x, torch.zeros(2, dtype=torch.complex128)))
    Host = dc.host_bfgs()
    A = torch.eye(5)
    A[0, 1] = 1e-3
    with pytest.raises(ValueError, match='symmetric'):
        Host((x,), H0=A)
    A[1, 0] = 1e-3 * (1 + 1e-9)                                             # asymmetric at rounding level: accepted
    assert torch.equal(Host((x,), H0=A).H, A)
    for bad in (torch.eye(4), torch.ones(5), torch.eye(5, dtype=torch.complex128), 'identity'):
        with pytest.raises(ValueError):
            Host((x,), H0=bad)
    assert torch.equal(Host((x,), H0=torch.tensor(0.5)).H, 0.5 * torch.eye(5)) and torch.equal(Host((x,)).H, torch.eye(5))
    with pytest.raises(ValueError, match='L0'):
        bfgs.FactoredInvHessian([torch.ones(5)], [torch.ones(5)], torch.ones(5), [1.0], H0=torch.ones(5))
    # LBFGS keeps refusing a dense tensor
    with pytest.raises(NotImplementedError, match='hmat'):
        import lbfgs_common as lc
        lc.host_lbfgs()((x,), H0=torch.eye(5))


def test_lbfgs_approx_cov_walks_the_groups_of_a_logprob(f64, monkeypatch):
    """the plumbing on the CPU, with the L-BFGS oracle of lbfgs_common in place of the kernels: one LBFGS per parameter group, the
    groups restored, a DiagMat of the right length whose pieces are the groups' _Hdiag"""
    import lbfgs_common as lc
    from bayeslim_amd import bfgs, hmat
    monkeypatch.setattr(bfgs.LBFGS, '_history_cls', lc.OracleHistory)
    prob, sizes = dc.quadratic_logprob('cpu')
    names = dict(prob._main_names)
    D = bfgs.lbfgs_approx_cov(prob, Nsteps=3, max_iter=2)
    assert isinstance(D, hmat.DiagMat) and D.diagonal().shape == (sum(sizes),)
    assert dict(prob._main_names) == names and prob.main_params.numel() == sum(sizes)
    want = dc.hdiag_by_hand(lc.host_lbfgs(), 'cpu', Nsteps=3, max_iter=2)
    assert torch.equal(D.diagonal(), want) and bool((want > 0).all()) and len(set(want.tolist())) == 2


def test_bfgs_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/bfgs.hip: no kernel has a private segment"""
    _, kernels, sizes = kernel_asm.read('bfgs')
    # 2 precisions x (matvec with 1 and 2 right-hand sides + rank2)
    assert len(kernels) == 6 and all('bfgs_' in k for k in kernels), kernels
    assert len(sizes) == 6 and max(sizes) == 0, sizes
