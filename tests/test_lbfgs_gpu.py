"""
GPU checks of the L-BFGS direction kernels (csrc/lbfgs.hip) and of bayeslim_amd/bfgs.py on them: rime_lbfgs_dots and
rime_lbfgs_combine against the float64 oracle of tests/lbfgs_common.py within its derived bounds, at the smallest shapes at
which each mechanism can break (a lone element, around a wave, a ragged tail, one element past a work-group's span, three
partials in the second reduction stage; one row, more rows than a wave's worth of anything, tables in wrapped order, rows
that are not 16-byte aligned), then two_loop_recursion, LBFGS.hvp and whole trajectories against the reference's record.
"""
import numpy as np
import pytest
import torch

import lbfgs_common as lc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = (torch.float32, torch.float64)
MS = (1, 2, 7, 33)


def sizes(dtype):
    from bayeslim_amd import bfgs
    span = bfgs.DOTS_SPAN[dtype]
    return (1, 63, 64, 65, 259, span + 1, 2 * span + 1)


def history(rng, m, N, dtype, offset=0):
    """m rows of S and of Y on the GPU; offset = 1 makes every row a view one element into its storage"""
    def one():
        buf = torch.empty(N + offset, dtype=dtype, device=DEV)
        buf[offset:] = torch.as_tensor(rng.normal(size=N)).to(dtype)
        return buf[offset:]
    return [one() for _ in range(m)], [one() for _ in range(m)]


def vector(rng, N, dtype, offset=0, positive=False):
    x = rng.uniform(0.5, 2.0, N) if positive else rng.normal(size=N)
    buf = torch.empty(N + offset, dtype=dtype, device=DEV)
    buf[offset:] = torch.as_tensor(x).to(dtype)
    return buf[offset:]


def hist_of(S, Y, d):
    from bayeslim_amd import bfgs
    h = bfgs._History(S[0].numel(), S[0].dtype, S[0].device, d)
    h.set_rows(S, Y)
    return h


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_dots_and_combine_against_the_oracle(dtype):
    rng = np.random.default_rng(11)
    worst_d = worst_c = 0.0
    for N in sizes(dtype):
        for m in MS:
            S, Y = history(rng, m, N, dtype)
            v = vector(rng, N, dtype)
            a, b = rng.normal(size=m), rng.normal(size=m)
            for d in (None, vector(rng, N, dtype, positive=True)):
                h = hist_of(S, Y, d)
                for k in sorted({-1, 0, m - 1, m // 2}):
                    kk = None if k < 0 else k
                    got = torch.as_tensor(h.dots(v, k))
                    want, sums = lc.oracle_dots(S, Y, v, d, kk), lc.oracle_dots_abs(S, Y, v, d, kk)
                    assert got.shape == want.shape == ((2, m) if k < 0 else (5, m))
                    q = lc.ratio(got - want, lc.dots_bound(N, dtype, sums))
                    worst_d = max(worst_d, q)
                    assert q <= 1.0, ('dots', N, m, d is not None, k, q)
                    if k >= 0:                                   # a row's first two results do not depend on k
                        assert torch.equal(got[:2], torch.as_tensor(h.dots(v)))
                r = h.combine(v, a, b, 0.7)
                assert r.dtype == dtype and r.shape == (N,)
                q = lc.ratio(r.cpu().double() - lc.oracle_combine(S, Y, v, d, a, b, 0.7),
                             lc.combine_bound(m, dtype, lc.oracle_combine_abs(S, Y, v, d, a, b, 0.7)))
                worst_c = max(worst_c, q)
                assert q <= 1.0, ('combine', N, m, d is not None, q)
    print('%s: worst error / bound  dots %.3f  combine %.3f' % (dtype, worst_d, worst_c))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_wrapped_table_and_misaligned_rows(dtype):
    """a table in rotated order over one (m, N) block (a ring that wrapped), and rows / v / d / the output's inputs that start
    one element into their storage: the element loads of the misaligned path read the same elements into the same registers
    as the 16-byte loads, so the results are BIT-IDENTICAL to the aligned ones (not merely within the bound)"""
    rng = np.random.default_rng(12)
    from bayeslim_amd import bfgs
    m = 7
    for N in (65, 259, bfgs.DOTS_SPAN[dtype] + 1):
        Sb = torch.as_tensor(rng.normal(size=(m, N))).to(dtype).to(DEV)
        Yb = torch.as_tensor(rng.normal(size=(m, N))).to(dtype).to(DEV)
        order = [3, 4, 5, 6, 0, 1, 2]
        S, Y = [Sb[i] for i in order], [Yb[i] for i in order]
        v, d = vector(rng, N, dtype), vector(rng, N, dtype, positive=True)
        a, b = rng.normal(size=m), rng.normal(size=m)
        h = hist_of(S, Y, d)
        got = torch.as_tensor(h.dots(v, 2))
        assert lc.ratio(got - lc.oracle_dots(S, Y, v, d, 2), lc.dots_bound(N, dtype, lc.oracle_dots_abs(S, Y, v, d, 2))) <= 1.0
        r = h.combine(v, a, b, 1.3)
        # the same values in separately allocated, aligned rows
        h2 = hist_of([t.clone() for t in S], [t.clone() for t in Y], d.clone())
        assert all(t.data_ptr() % 16 == 0 for t in h2.s + h2.y)
        assert torch.equal(got, torch.as_tensor(h2.dots(v.clone(), 2))) and torch.equal(r, h2.combine(v.clone(), a, b, 1.3))
        # and one element into their storage
        def shifted(t):
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
            buf[1:] = t
            return buf[1:]
        S3, Y3, v3, d3 = [shifted(t) for t in S], [shifted(t) for t in Y], shifted(v), shifted(d)
        assert all(t.data_ptr() % 16 != 0 for t in S3 + Y3 + [v3, d3])
        h3 = hist_of(S3, Y3, d3)
        assert torch.equal(got, torch.as_tensor(h3.dots(v3, 2))) and torch.equal(r, h3.combine(v3, a, b, 1.3))
        # a mixture: only some rows misaligned
        h4 = hist_of(S3[:3] + S[3:], Y[:5] + Y3[5:], d)
        assert torch.equal(got, torch.as_tensor(h4.dots(v3, 2))) and torch.equal(r, h4.combine(v, a, b, 1.3))


def test_complex_parameters_through_the_real_views():
    from bayeslim_amd import bfgs
    g = lc.golden()
    s, y, vec, d, ref = [g['tlrc_' + k].to(DEV) for k in ('s', 'y', 'vec', 'diag', 'out')]
    r = bfgs.two_loop_recursion(vec, list(s), list(y), g['tlrc_rho'], d)
    assert r.is_complex() and r.shape == ref.shape
    assert float((r - ref).abs().max() / ref.abs().max()) <= lc.FACTOR * lc.TLR_RESTATEMENT
    x = torch.zeros_like(vec).requires_grad_(True)
    opt = bfgs.LBFGS((x,), H0=d, history_size=10, update_Hdiag=False)
    for si, yi in zip(s, y):
        opt.update_hessian(si, yi)
    r = opt.hvp(vec)
    assert float((r - ref).abs().max() / ref.abs().max()) <= lc.FACTOR * lc.TLR_RESTATEMENT
    assert torch.equal(opt._Hdiag, torch.ones_like(d))
    # complex64: the dtype plumbing only (the float32 arithmetic is bounded where the kernels are tested on their own)
    r32 = bfgs.two_loop_recursion(vec.to(torch.complex64), list(s.to(torch.complex64)), list(y.to(torch.complex64)), g['tlrc_rho'],
                                  d.float())
    assert r32.dtype == torch.complex64 and r32.shape == ref.shape and bool(torch.isfinite(torch.view_as_real(r32)).all())


@pytest.mark.parametrize('N,m,kind', lc.tlr_cases())
def test_two_loop_recursion_and_hvp_against_the_reference(N, m, kind):
    """float64 on the GPU against the recorded outputs, with the constant and factor of the host test"""
    from bayeslim_amd import bfgs
    s, y, vec, rho, H0, ref = [t.to(DEV) for t in lc.tlr_inputs(lc.golden(), N, m, kind)]
    r = bfgs.two_loop_recursion(vec, list(s), list(y), list(rho), H0)
    e1 = float((r - ref).abs().max() / ref.abs().max())
    x = torch.zeros(N, dtype=torch.float64, device=DEV, requires_grad=True)
    opt = bfgs.LBFGS((x,), H0=H0, history_size=m, update_Hdiag=False)
    for si, yi in zip(s, y):
        opt.update_hessian(si, yi, alpha=1.0)
    assert len(opt._s) == m
    e2 = float((opt.hvp(vec) - ref).abs().max() / ref.abs().max())
    print('tlr_%d_%d_%s: two_loop_recursion %.3e hvp %.3e' % (N, m, kind, e1, e2))
    assert e1 <= lc.FACTOR * lc.TLR_RESTATEMENT and e2 <= lc.FACTOR * lc.TLR_RESTATEMENT


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_fused_update_equals_separate_update_and_hvp_and_is_reproducible(dtype):
    """one dots launch for the new pair AND the next gradient (what step() does) against update_hessian followed by hvp:
    identical bits, through a ring that wraps and a rejected pair; and the same direction twice: identical bits.  N spans
    three work-groups of the dots pass."""
    from bayeslim_amd import bfgs
    rng = np.random.default_rng(13)
    N, hs = 2 * bfgs.DOTS_SPAN[dtype] + 1, 3
    d = vector(rng, N, dtype, positive=True)
    mk = lambda: bfgs.LBFGS((torch.zeros(N, dtype=dtype, device=DEV, requires_grad=True),), H0=d, history_size=hs)
    A, B = mk(), mk()
    for i in range(hs + 3):
        s = vector(rng, N, dtype)
        y = -s if i == hs + 1 else s * vector(rng, N, dtype, positive=True)
        grad = vector(rng, N, dtype)
        dots = A._update(s, y, 1.0, bfgs._real_view(grad))
        pa = A._direction(grad, dots)
        B.update_hessian(s, y, alpha=1.0)
        pb = B.hvp(grad)
        assert torch.equal(pa, pb), i
        assert torch.equal(pb, B.hvp(grad)) and torch.equal(pa, A.hvp(grad)), i
        assert A._gamma == B._gamma and np.array_equal(A._SY, B._SY) and np.array_equal(A._YDY, B._YDY)
        assert len(A._s) == len(B._s) == min(i + 1, hs)
    assert bool(torch.isfinite(pa).all())


@pytest.mark.parametrize('kind', lc.TRAJ_KINDS)
def test_trajectory_against_the_reference(kind):
    """bfgs.LBFGS in float64 on the GPU on the reference's recorded trajectories: exit code, func_evals, n_iter and pair count
    equal, losses per step, final parameters, _Hdiag and _rho within FACTOR x the recorded discrepancy of the restatement;
    the inner products step() kept for the next direction are those of a fresh launch"""
    from bayeslim_amd import bfgs
    g = lc.golden()
    icov, x0, H0 = lc.traj_problem(g)
    res, opt = lc.run_trajectory(bfgs.LBFGS, icov, x0, H0, kind, device=DEV)
    e = lc.traj_discrepancy(res, g, kind)
    print('trajectory %s on the GPU: %.3e' % (kind, e))
    assert e <= lc.FACTOR * lc.TRAJ_RESTATEMENT
    assert len(opt._s) == len(opt._y) == lc.TRAJ['history_size']
    grad, dots = opt._pending
    assert grad is opt._flat_grad
    fresh = opt._hist.dots(bfgs._real_view(grad))
    assert np.array_equal(fresh[0], dots[0]) and np.array_equal(fresh[1], dots[1])
    assert torch.equal(opt.hvp(grad), opt._direction(grad, dots))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_ring_wrap_and_rejected_pair(dtype):
    """more accepted pairs than history_size: the newest history_size survive and hvp is the oracle's two-loop recursion over
    exactly those (within the composed dots / combine bounds for float32: asserted against a float64 run of the same class
    on the oracle); a pair with y . s <= tolerance_grad changes nothing"""
    from bayeslim_amd import bfgs
    rng = np.random.default_rng(14)
    N, hs = 259, 4
    d = vector(rng, N, dtype, positive=True)
    opt = bfgs.LBFGS((torch.zeros(N, dtype=dtype, device=DEV, requires_grad=True),), H0=d, history_size=hs)
    pairs = []
    for i in range(hs + 3):
        s = vector(rng, N, dtype)
        y = s * vector(rng, N, dtype, positive=True)
        opt.update_hessian(s, y, alpha=float(i))
        pairs.append((s, y))
        assert len(opt._s) == len(opt._y) == len(opt._rho) == len(opt._alpha) == min(i + 1, hs)
    assert opt._alpha == [3.0, 4.0, 5.0, 6.0]
    assert all(a is p[0] for a, p in zip(opt._s, pairs[-hs:])) and all(a is p[1] for a, p in zip(opt._y, pairs[-hs:]))
    SY, YDY, gam, rho = opt._SY.copy(), opt._YDY.copy(), opt._gamma, list(opt._rho)
    s = vector(rng, N, dtype)
    opt.update_hessian(s, -s)
    opt.update_hessian(s, torch.zeros_like(s))
    assert len(opt._s) == hs and opt._rho == rho and opt._gamma == gam
    assert np.array_equal(opt._SY, SY) and np.array_equal(opt._YDY, YDY)
    assert all(a is p[0] for a, p in zip(opt._s, pairs[-hs:]))
    vec = vector(rng, N, dtype)
    S, Y = [p[0] for p in pairs[-hs:]], [p[1] for p in pairs[-hs:]]
    want = lc.oracle_two_loop(vec, S, Y, [1.0 / float(lc._w(a) @ lc._w(b)) for a, b in zip(S, Y)],
                              float(lc._w(S[-1]) @ lc._w(Y[-1])) / float(lc._w(Y[-1]) @ (lc._w(d) * lc._w(Y[-1]))), d)
    got = opt.hvp(vec).cpu().double()
    e = float((got - want).abs().max() / want.abs().max())
    print('%s: hvp after the wrap against the oracle two-loop recursion %.3e' % (dtype, e))
    if dtype == torch.float64:
        assert e <= lc.FACTOR * lc.TLR_RESTATEMENT
    else:
        # float32: the kernels' part is the bounds of lbfgs_common on the operations themselves -- the inner products
        # within dots_bound, and the combination of the coefficients they give within combine_bound
        h = opt._hist
        o = torch.as_tensor(h.dots(bfgs._real_view(vec)))
        assert lc.ratio(o - lc.oracle_dots(S, Y, vec, d), lc.dots_bound(N, dtype, lc.oracle_dots_abs(S, Y, vec, d))) <= 1.0
        a, b = bfgs.compact_coeffs(opt._SY, opt._YDY, o[0].numpy(), o[1].numpy(), opt._gamma)
        assert lc.ratio(got - lc.oracle_combine(S, Y, vec, d, a, b, opt._gamma),
                        lc.combine_bound(hs, dtype, lc.oracle_combine_abs(S, Y, vec, d, a, b, opt._gamma))) <= 1.0
