"""
CPU-side checks of the optimiser layer (bayeslim_amd/bfgs.py, rime_lbfgs_dots, rime_lbfgs_combine): the compact-form
recurrence, cubic_interpolate and strong_wolfe against the reference's recorded results (tests/golden/bfgs.npz), the restated
step() on the float64 oracle of tests/lbfgs_common.py against the recorded trajectories, argument validation without a GPU,
the workspace size, and the no-scratch property of the built kernels.
"""
import ctypes

import numpy as np
import pytest
import torch

import lbfgs_common as lc
import kernel_asm


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def rel(r, ref):
    return float((r - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('N,m,kind', lc.tlr_cases())
def test_compact_coeffs_reproduces_the_two_loop_recursion(f64, N, m, kind):
    """float64 Gram matrices of the fixture + compact_coeffs + the float64 combine against the reference's output, within
    FACTOR x the recorded discrepancy of this very restatement (lbfgs_common.TLR_RESTATEMENT); with the recorded rho and with
    rho = 1 / diag(SY), and the oracle's own two-loop recursion as a cross-check of the fixture"""
    from bayeslim_amd import bfgs
    s, y, vec, rho, H0, ref = lc.tlr_inputs(lc.golden(), N, m, kind)
    gam, d = (float(H0), None) if kind == 'scalar' else (1.0, H0)
    SY, YDY = lc.gram(list(s), list(y), d)
    o = lc.oracle_dots(list(s), list(y), vec, d).numpy()
    for r_ in (rho, None):
        a, b = bfgs.compact_coeffs(SY, YDY, o[0], o[1], gam, rho=r_)
        e = rel(lc.oracle_combine(list(s), list(y), vec, d, a, b, gam), ref)
        print('tlr_%d_%d_%s rho %s: %.3e' % (N, m, kind, 'given' if r_ is not None else 'diag', e))
        assert e <= lc.FACTOR * lc.TLR_RESTATEMENT
    assert rel(lc.oracle_two_loop(vec, list(s), list(y), rho, gam, d), ref) <= lc.FACTOR * lc.TLR_RESTATEMENT


def test_compact_coeffs_complex_through_the_real_views(f64):
    from bayeslim_amd import bfgs
    g = lc.golden()
    s, y, vec, d = lc.realify(g['tlrc_s']), lc.realify(g['tlrc_y']), lc.realify(g['tlrc_vec']), g['tlrc_diag'].repeat_interleave(2)
    SY, YDY = lc.gram(list(s), list(y), d)
    o = lc.oracle_dots(list(s), list(y), vec, d).numpy()
    a, b = bfgs.compact_coeffs(SY, YDY, o[0], o[1], 1.0, rho=g['tlrc_rho'])
    r = torch.view_as_complex(lc.oracle_combine(list(s), list(y), vec, d, a, b, 1.0).reshape(-1, 2))
    assert rel(r, g['tlrc_out']) <= lc.FACTOR * lc.TLR_RESTATEMENT


def test_cubic_interpolate_against_the_reference(f64):
    from bayeslim_amd import bfgs
    g = lc.golden()
    for i, row in enumerate(lc.CUBIC_ARGS):
        bounds = None if np.isnan(row[6]) else (row[6], row[7])
        want = float(g['cubic_out'][i])
        got_t = float(bfgs.cubic_interpolate(*[torch.tensor(v) for v in row[:6]], bounds=bounds))
        got_f = float(bfgs.cubic_interpolate(*row[:6], bounds=bounds))
        sqrt = (row[2] + row[5] - 3 * (row[1] - row[4]) / (row[0] - row[3])) ** 2 - row[2] * row[5] >= 0
        tol = 1e-14 * abs(want) if sqrt else 0.0
        assert abs(got_t - want) <= tol and abs(got_f - want) <= tol, (i, got_t, got_f, want)
    assert sum(1 for r in lc.CUBIC_ARGS if (r[2] + r[5] - 3 * (r[1] - r[4]) / (r[0] - r[3])) ** 2 - r[2] * r[5] < 0) == 2


@pytest.mark.parametrize('name', ['newton', 'quartic'])
def test_strong_wolfe_against_the_reference(f64, name):
    """the same arithmetic in the same order: loss, step, evaluation count and gradient equal the recorded ones"""
    from bayeslim_amd import bfgs
    g = lc.golden()
    f, x0, p, alpha0, c2 = lc.wolfe_objective(name)
    loss, grad = f(x0)
    f_new, g_new, alpha, n = bfgs.strong_wolfe(lc.wolfe_obj_func(f), x0, alpha0, p, float(loss), grad, grad @ p, c1=1e-4, c2=c2,
                                               tolerance_change=1e-9, max_ls=25)
    want = g['wolfe_%s_scalars' % name]
    assert n == int(want[2]) == (1 if name == 'newton' else 5)
    assert float(f_new) == float(want[0]) and float(alpha) == float(want[1])
    assert torch.equal(g_new, g['wolfe_%s_grad' % name])


@pytest.mark.parametrize('kind', lc.TRAJ_KINDS)
def test_restated_step_reproduces_the_reference_trajectory(f64, kind):
    """bfgs.LBFGS.step on the float64 oracle (compact_coeffs + torch dot products, no kernel): exit code, func_evals, n_iter
    and pair count equal, the floating-point record within FACTOR x lbfgs_common.TRAJ_RESTATEMENT"""
    g = lc.golden()
    icov, x0, H0 = lc.traj_problem(g)
    res, opt = lc.run_trajectory(lc.host_lbfgs(), icov, x0, H0, kind)
    e = lc.traj_discrepancy(res, g, kind)
    print('trajectory %s: %.3e' % (kind, e))
    assert e <= lc.FACTOR * lc.TRAJ_RESTATEMENT
    assert len(opt._s) == len(opt._y) == len(opt._rho) == len(opt._alpha) == lc.TRAJ['history_size'] and opt.n_iter == 12


def test_rejected_pair_and_ring_wrap_on_the_oracle(f64):
    """a pair without curvature leaves history, Gram matrices and gamma alone; the ring keeps the newest history_size pairs
    and hvp is the two-loop recursion over exactly those"""
    rng = np.random.default_rng(5)
    N, hs = 23, 3
    x = torch.zeros(N, requires_grad=True)
    d = torch.as_tensor(rng.uniform(0.5, 2.0, N))
    opt = lc.host_lbfgs()((x,), H0=d.clone(), history_size=hs)
    pairs = []
    for i in range(hs + 2):
        s = torch.as_tensor(rng.normal(size=N))
        y = s * torch.as_tensor(rng.uniform(0.5, 2.0, N))
        opt.update_hessian(s, y, alpha=0.5 + i)
        pairs.append((s, y))
        assert len(opt._s) == min(i + 1, hs)
    assert opt._alpha == [2.5, 3.5, 4.5]
    SY, YDY, gam, rho = opt._SY.copy(), opt._YDY.copy(), opt._gamma, list(opt._rho)
    s = torch.as_tensor(rng.normal(size=N))
    opt.update_hessian(s, -s, alpha=9.0)                                   # y . s < 0
    opt.update_hessian(s, torch.zeros(N), alpha=9.0)                       # y . s = 0
    assert len(opt._s) == hs and opt._rho == rho and opt._gamma == gam and opt._alpha == [2.5, 3.5, 4.5]
    assert np.array_equal(opt._SY, SY) and np.array_equal(opt._YDY, YDY)
    assert all(a is b[0] for a, b in zip(opt._s, pairs[-hs:])) and all(a is b[1] for a, b in zip(opt._y, pairs[-hs:]))
    vec = torch.as_tensor(rng.normal(size=N))
    want = lc.oracle_two_loop(vec, [p[0] for p in pairs[-hs:]], [p[1] for p in pairs[-hs:]], rho, gam, d)
    assert rel(opt.hvp(vec), want) <= lc.FACTOR * lc.TLR_RESTATEMENT
    ys, ydy = float(pairs[-1][0] @ pairs[-1][1]), float(pairs[-1][1] @ (d * pairs[-1][1]))
    assert abs(gam - ys / ydy) <= 1e-15 * gam and torch.allclose(opt._Hdiag, gam * d, rtol=1e-15, atol=0)


def test_entry_points_reject_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)      # non-null dummy; never dereferenced on a rejected call
    big = 1 << 30

    def dots(dtype=0, S=one, Y=one, m=3, N=100, v=one, d=None, k=-1, out=one, ws=one, nbytes=big):
        return lib.rime_lbfgs_dots(dtype, S, Y, m, N, v, d, k, out, ws, nbytes, None)

    def comb(dtype=0, S=one, Y=one, m=3, N=100, v=one, d=None, a=one, b=one, gamma=1.0, r=one):
        return lib.rime_lbfgs_combine(dtype, S, Y, m, N, v, d, a, b, gamma, r, None)

    for f in (dots, comb):
        assert f(dtype=2) == -1 and f(dtype=-1) == -1                       # unknown dtype
        assert f(m=0) == -1 and f(m=-4) == -1 and f(N=0) == -1 and f(N=-1) == -1
        assert f(S=None) == -1 and f(Y=None) == -1 and f(v=None) == -1      # null tables, null vector
    assert dots(out=None) == -1 and comb(a=None) == -1 and comb(b=None) == -1 and comb(r=None) == -1
    assert dots(k=3) == -1 and dots(k=-2) == -1 and dots(k=100) == -1       # k outside [-1, m)
    need = lib.rime_lbfgs_workspace(3, 100)
    assert need > 0
    assert dots(nbytes=need - 1) == -2 and dots(ws=None) == -2 and dots(k=2, nbytes=0) == -2
    assert dots(m=0, nbytes=0) == -1                                        # the arguments are judged before the workspace


def test_workspace_is_monotone():
    from bayeslim_amd._lib import lib
    from bayeslim_amd import bfgs
    w = lib.rime_lbfgs_workspace
    Ns = [1, 63, 2048, 2049, 4096, 4097, 10 ** 5, 10 ** 7, 5 * 10 ** 7, 10 ** 10]
    ms = [1, 2, 7, 33, 100, 129, 1000]
    for m in ms:
        sizes = [w(m, N) for N in Ns]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] == m * 5 * 8
    for N in Ns:
        sizes = [w(m, N) for m in ms]
        assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert w(0, 10) == 0 and w(3, 0) == 0
    # one partial per work-group of the float64 span, at most 1024 of them
    assert w(1, bfgs.DOTS_SPAN[torch.float64] + 1) == 2 * 40 and w(100, 5 * 10 ** 7) == 1024 * 100 * 40


def test_cpu_tensors_raise(f64):
    from bayeslim_amd import bfgs
    x = torch.zeros(5, requires_grad=True)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        bfgs.LBFGS((x,))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        bfgs.two_loop_recursion(torch.zeros(5), [torch.ones(5)], [torch.ones(5)], [0.2])
    with pytest.raises(NotImplementedError, match='hmat'):
        lc.host_lbfgs()((x,), H0=torch.eye(5))
    with pytest.raises(NotImplementedError, match='hmat'):
        lc.host_lbfgs()((x,), H0=object())
    import bayeslim_amd
    assert bayeslim_amd.bfgs is bfgs


def test_lbfgs_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/lbfgs.hip: no kernel has a private segment"""
    _, kernels, sizes = kernel_asm.read('lbfgs')
    # 2 precisions x (dots with and without a new pair + combine) + the second reduction stage
    assert len(kernels) == 7 and all('lbfgs_' in k for k in kernels), kernels
    assert len(sizes) == 7 and max(sizes) == 0, sizes
