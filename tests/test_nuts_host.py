"""
CPU-side checks of the No-U-Turn sampler layer (bayeslim_amd/nuts.py, rime_nuts_leaf_open / rime_nuts_leaf_close): the numpy
restatement of tests/nuts_common.py against the reference's recorded chains (tests/golden/nuts.npz) with its recorded constant,
the long-double restatement of the two kernels against exact rational arithmetic, the argument checks of the entry points
(before any HIP call, so they run without a GPU), what the sampler refuses, and the gfx950 assembly of this build.
"""
import ctypes
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import hmc_common as hc
import kernel_asm
import nuts_common as nc


# --------------------------------------------------------------------------------------------- the restatement and the record
@pytest.mark.parametrize('tag', list(nc.CHAINS))
def test_oracle_reproduces_the_recorded_chain(tag):
    """every decision of the reference (accept, restart, depth, fn_evals, directions, leaves, every uniform draw) and its
    floating-point record within the recorded constant"""
    g = nc.golden()
    recs = nc.run_oracle_chain(g, tag)
    e = nc.chain_discrepancy(recs, g, tag)
    print('OracleNUTS against chain %s: %.3e' % (tag, e))
    assert e <= nc.NUTS_RESTATEMENT
    assert [len(r['leaf_K']) for r in recs] == [int(n) - 1 for n in g['chain_%s_fn_evals' % tag]]    # one evaluation per leaf and move
    if nc.CHAINS[tag]['track_states']:
        assert [len(r['states']) for r in recs] == g['chain_%s_nstates' % tag].tolist()
        assert all(len(r['states']) == 2 ** r['depth'] for r in recs)                  # the leaves of the base tree and the start


def test_the_record_is_decisive():
    """what the generator asserted, read back from the file: the tests that compare decisions compare something"""
    g = nc.golden()
    a, c = nc.CHAINS['a'], nc.CHAINS['c']
    assert g['chain_a_depth'].max() == a['max_tree_depth'] and g['chain_a_depth'].min() < a['max_tree_depth']
    assert {-1.0, 1.0} <= set(g['chain_a_dirs'].ravel()) and set(g['chain_a_accept']) == {0.0, 1.0}
    assert set(g['chain_b_dirs'].ravel()) == {1.0} and g['chain_b_nstates'].min() > 1
    assert g['chain_c_restart'].any() and not g['chain_c_restart'][0]
    dH = g['chain_c_leaf_H'] - g['chain_c_H_start'][:, None]
    late = [(np.nanmax(dH[i]) > c['dHmax']) and g['chain_c_depth'][i] >= 2 and not g['chain_c_restart'][i] for i in range(nc.STEPS)]
    assert any(late)
    assert not g['chain_c_restart'].all() and np.isnan(g['chain_c_H'][g['chain_c_restart'] > 0]).all()
    for tag in nc.CHAINS:
        dH = g['chain_%s_leaf_H' % tag] - g['chain_%s_H_start' % tag][:, None]
        assert np.nanmin(np.abs(dH - nc.CHAINS[tag]['dHmax'])) > nc.MARGIN


def test_kernel_restatement_is_exact_enough():
    """oracle_open / oracle_close in long double against rational arithmetic on the rounded operands, and the zero rule"""
    rng = np.random.default_rng(5)
    n = 9
    q0, p0, g0, g1, eps, c, qf, pf = [rng.normal(size=n).astype(np.float32) for _ in range(8)]
    h = -0.37
    q1, p1 = nc.oracle_open(q0, p0, g0, eps, c, h, np.float32)
    fr = lambda x: F(float(x))
    hk, hd = fr(np.float32(h / 2)), fr(np.float32(h))
    for i in range(n):
        pe = fr(p0[i]) - hk * fr(eps[i]) * fr(g0[i])
        qe = fr(q0[i]) + hd * fr(eps[i]) * fr(c[i]) ** 2 * pe
        assert abs(float(F(float(p1[i])) - pe)) <= 1e-15 * (abs(float(p0[i])) + abs(float(pe)))
        assert abs(float(F(float(q1[i])) - qe)) <= 1e-15 * (abs(float(q0[i])) + abs(float(qe)))
    q1r, p1r = q1.astype(np.float32), p1.astype(np.float32)
    p2, (E, far, near) = nc.oracle_close(q1r, p1r, g1, eps, c, h, qf, pf, np.float32)
    pe = [fr(p1r[i]) - hk * fr(eps[i]) * fr(g1[i]) for i in range(n)]
    want = (sum((fr(c[i]) * pe[i]) ** 2 for i in range(n)) / 2, sum((fr(q1r[i]) - fr(qf[i])) * fr(pf[i]) for i in range(n)),
            sum((fr(q1r[i]) - fr(qf[i])) * pe[i] for i in range(n)))
    scale = (want[0], sum(abs((fr(q1r[i]) - fr(qf[i])) * fr(pf[i])) for i in range(n)), sum(abs((fr(q1r[i]) - fr(qf[i])) * pe[i]) for i in range(n)))
    for got, w, s in zip((E, far, near), want, scale):
        assert abs(float(got) - float(w)) <= 1e-14 * float(s)
    assert nc.oracle_close(q1r, p1r, g1, eps, c, h, None, None, np.float32)[1][1:] == (None, None)
    # a span of zero: the bounds are zero and ask for the exact value
    Bp = hc.p_bound(p1r, g1, eps, h / 2, np.float32)
    assert nc.dots_bound(q1r, q1r, pf, p2, Bp, np.float32) == (0.0, 0.0)
    assert nc.within(0.0, 0.0, 0.0) and not nc.within(1e-300, 0.0, 0.0) and nc.within(1.0, 1.0 + 1e-9, 1e-8)
    B = nc.dots_bound(q1r, qf, pf, p2, Bp, np.float32)
    assert 0 < B[0] < 1e-4 * float(scale[1]) and 0 < B[1] < 1e-4 * float(scale[2])
    # the angles of the restatement of the move: the reference's signs for either direction
    d = lambda x: {'k': np.asarray(x, dtype=float)}
    (minus, plus), _ = nc.angles(d([0, 0]), d([1, 0]), d([1, 1]), d([0, 2]), 1.0)
    assert (minus, plus) == (1.0, 2.0)
    (minus, plus), _ = nc.angles(d([0, 0]), d([1, 0]), d([1, 1]), d([0, 2]), -1.0)      # far is now q_plus: the span is far - leaf
    assert (minus, plus) == (-2.0, -1.0)


# ---------------------------------------------------------------------------------------------------------- the entry points
def test_entry_points_reject_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    P = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]      # distinct non-null dummies 4096 bytes apart; never dereferenced
    big = 1 << 20
    nan = float('nan')

    def opn(dtype=0, N=100, q0=P[0], p0=P[1], g0=P[2], q1=P[3], p1=P[4], eps=None, c=None, h=0.5):
        return lib.rime_nuts_leaf_open(dtype, N, q0, p0, g0, q1, p1, eps, c, h, None)

    def cls(dtype=0, N=100, q1=P[0], p1=P[1], g1=P[2], eps=None, c=None, h=0.5, q_far=P[3], p_far=P[4], out=P[5], ws=P[6], nbytes=big):
        return lib.rime_nuts_leaf_close(dtype, N, q1, p1, g1, eps, c, h, q_far, p_far, out, ws, nbytes, None)

    for call in (opn, cls):
        assert call(dtype=2) == -1 and call(dtype=-1) == -1                      # unknown dtype
        assert call(N=-1) == -1 and call(N=-(1 << 40)) == -1
        assert call(h=nan) == -1 and call(h=0.0) == -1 and call(h=-0.0) == -1
        assert call(h=1e-60) == -1 and call(h=-1e-60) == -1                      # half of it rounds to zero in float32
        assert call(dtype=1, h=5e-324) == -1                                     # and in float64
    for name in ('q0', 'p0', 'g0', 'q1', 'p1'):
        assert opn(**{name: None}) == -1, name
    for name in ('q1', 'p1', 'g1', 'out'):
        assert cls(**{name: None}) == -1, name
    assert cls(q_far=None) == -1 and cls(p_far=None) == -1                       # only one of the pair
    # open is out of place: q1 or p1 on an input, overlapping one by a single element, or on each other
    for i in range(3):
        assert opn(q1=P[i]) == -1 and opn(p1=P[i]) == -1
    assert opn(eps=P[5], q1=P[5]) == -1 and opn(c=P[5], p1=P[5]) == -1 and opn(q1=P[3], p1=P[3]) == -1
    assert opn(N=1024, q1=ctypes.c_void_p(P[0].value + 4092)) == -1              # the last element of q0
    assert opn(N=1024, q1=ctypes.c_void_p(P[0].value - 4092)) == -1
    assert opn(N=1025, dtype=0) == -1                                            # neighbours 4096 bytes apart now overlap
    need = lib.rime_nuts_workspace(100)
    assert need == 3 * lib.rime_hmc_workspace(100) > 0
    assert cls(nbytes=need - 1) == -2 and cls(ws=None) == -2 and cls(q_far=None, p_far=None, nbytes=need - 1) == -2
    assert cls(N=-1, nbytes=0) == -1 and cls(h=nan, ws=None) == -1               # the arguments are judged before the workspace
    assert cls(h=1e-60, ws=None) == -2 and cls(dtype=7, h=1e-60, ws=None) == -1  # ... the rounding of h after it, as rime_hmc_step
    assert lib.rime_nuts_workspace(-1) == 0
    Ns = [0, 1, 2048, 2049, 10 ** 5, 10 ** 7, 10 ** 10]
    assert [lib.rime_nuts_workspace(N) for N in Ns] == [3 * lib.rime_hmc_workspace(N) for N in Ns]


def test_entry_points_remaining_return_paths():
    """the size bound, every pair of an output with an input of open, and the step whose half is zero: in float64, of either sign,
    and against the workspace of close"""
    from bayeslim_amd._lib import lib
    P = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]
    bound = 0x3fffffffffffffff                                                   # the largest N the entry points take

    def opn(dtype=0, N=100, q0=P[0], p0=P[1], g0=P[2], q1=P[3], p1=P[4], eps=None, c=None, h=0.5):
        return lib.rime_nuts_leaf_open(dtype, N, q0, p0, g0, q1, p1, eps, c, h, None)

    def cls(dtype=0, N=100, h=0.5, ws=P[6], nbytes=1 << 20):
        return lib.rime_nuts_leaf_close(dtype, N, P[0], P[1], P[2], None, None, h, P[3], P[4], P[5], ws, nbytes, None)

    assert opn(N=bound + 1) == -1 and cls(N=bound + 1) == -1 and opn(N=1 << 62, dtype=1) == -1
    assert lib.rime_nuts_workspace(bound + 1) == 0 and lib.rime_hmc_workspace(bound + 1) == 0 and lib.rime_hmc_workspace(-1) == 0
    ins = dict(q0=0, p0=1, g0=2, eps=5, c=6)
    for out in ('q1', 'p1'):
        for name, i in ins.items():
            assert opn(**{name: P[i], out: P[i]}) == -1, (out, name)                                  # the same buffer
            assert opn(**{name: P[i], out: ctypes.c_void_p(P[i].value + 396)}) == -1, (out, name)    # its last element
            assert opn(**{name: P[i], out: ctypes.c_void_p(P[i].value - 396)}) == -1, (out, name)
    assert opn(p1=ctypes.c_void_p(P[3].value + 396)) == -1                       # the two outputs share one element
    for dtype in (0, 1):
        for h in (5e-324, -5e-324):                                              # h / 2 is zero in float64 already
            assert opn(dtype=dtype, h=h) == -1 and cls(dtype=dtype, h=h) == -1
            assert cls(dtype=dtype, h=h, ws=None) == -2 and cls(dtype=dtype, h=h, nbytes=0) == -2     # ... judged after the workspace
    assert opn(h=1e-46) == -1 and cls(h=-1e-46) == -1                            # float32: half of it is below the smallest subnormal


# ------------------------------------------------------------------------------------------------------- what the sampler refuses
def test_nuts_names_what_it_does_not_provide_and_has_no_cpu_path():
    import bayeslim_amd
    from bayeslim_amd import nuts, sampler
    from bayeslim_amd.paramdict import ParamDict
    assert bayeslim_amd.nuts is nuts and issubclass(nuts.NUTS, sampler.HMC) and nuts.NUTS is not sampler.NUTS
    x = ParamDict({'a': torch.zeros(4, 3), 'b': torch.zeros(5)})
    pot = lambda x: (torch.tensor(0.0), x * 0)
    eye = ParamDict({'a': torch.eye(12), 'b': torch.eye(5)})

    def refuses(match, eps=0.1, **kw):
        with pytest.raises(NotImplementedError, match=match):
            nuts.NUTS(pot, x, eps, **kw)

    refuses('diag_mass=False', diag_mass=False)
    refuses('hmat', cov_L=eye)
    refuses('hmat', hess_L=torch.eye(5))
    refuses('pmask', pmask={'a': torch.ones(4, 3), 'b': torch.ones(5)})
    refuses('StepSize', eps=ParamDict({'a': torch.ones(4, 3, dtype=torch.complex64), 'b': torch.ones(5)}))
    with pytest.raises(TypeError):
        nuts.NUTS(pot, x, 0.1, Nstep=3)                                          # the reference's constructor has no Nstep
    for word in ('DynamicStepSize', 'StepSize', 'RecycledHMC', 'Betancourt', 'dense', 'pmask', 'complex step sizes'):
        assert word in nuts.__doc__, word
    assert 'bayeslim_amd.nuts' in sampler.__doc__
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        nuts.NUTS(pot, x, 0.1)
    v = lambda: torch.zeros(5)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        nuts.leaf_open(v(), v(), v(), v(), v(), None, None, 0.5)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        nuts.leaf_close(v(), v(), v(), None, None, 0.5, v(), v(), torch.zeros(3, dtype=torch.float64))
    fields = ('q_left', 'p_left', 'grad_left', 'q_right', 'p_right', 'grad_right', 'q_prop', 'p_prop', 'q_prop_U', 'q_prop_H',
              'weight', 'turning', 'diverging', 'states')

    class S:
        qv, pv, gv = 'q', 'p', 'g'
    t = nuts.TreeInfo(S, S, S, 1.0, 2.0, -2.0)
    assert all(hasattr(t, f) for f in fields) and (t.q_left, t.p_right, t.grad_left, t.q_prop) == ('q', 'p', 'g', 'q')
    assert (t.turning, t.diverging, t.states) == (False, False, None)
    assert abs(nuts._logaddexp(-3.0, -1.0) - np.logaddexp(-3.0, -1.0)) < 1e-15 and nuts._logaddexp(-1.0, -3.0) == nuts._logaddexp(-3.0, -1.0)


def test_nuts_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/nuts.hip: no kernel has a private segment"""
    asm, kernels, sizes = kernel_asm.read('nuts')
    # open in 2 precisions, close in 2 precisions with and without the projections, the second reduction stage
    assert len(kernels) == 7 and all('nuts_leaf_' in k for k in kernels), kernels
    assert len(sizes) == 7 and max(sizes) == 0, sizes
