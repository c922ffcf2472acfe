"""
CPU-side checks of the mutual-coupling term (calibration.VisCoupling, ops.CouplingPlan, rime_coupling_*): the float64
restatement of tests/coupling_common.py against the reference's recorded outputs and gradients (tests/golden/coupling.npz)
within the derived bound, setup_coupling against the recorded index attributes and delay phasors, the ValueError cases, the
plan tables on crafted inputs, argument validation of the entry points without a GPU, the workspace query and module
bookkeeping.
"""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

import coupling_common as cc

RECORDED = sorted(k[2:] for k in cc.golden() if k.startswith('W_'))


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def golden_module(tb=False, dtype=torch.float64, **kw):
    """(VisCoupling on the CPU, bls) of the fixture; only the host side of it can run here"""
    from bayeslim_amd import calibration
    g = cc.golden()
    ants, bls = [int(a) for a in g['ants']], [tuple(int(x) for x in b) for b in g['bls']]
    antpos = {a: torch.as_tensor(v) for a, v in zip(ants, g['antvecs'])}
    p = torch.as_tensor(g['p_tb' if tb else 'p_pt']).to(dtype)
    R = calibration.VisModelResponse(param_type='com', times=torch.as_tensor(g['times']) if not tb else None)
    m = calibration.VisCoupling(p, torch.as_tensor(g['freqs']), antpos, bls, R=R, **kw)
    return m, bls


@pytest.mark.parametrize('tag', RECORDED)
def test_restatement_reproduces_the_reference(tag):
    g = cc.golden()
    (W, gd, gx), (bw, bd, bx) = cc.golden_bounds(tag)
    gp = g['gp_' + tag]
    ratios = (cc.ratio(W, g['W_' + tag][0, 0], bw), cc.ratio(gd, g['gd_' + tag][0, 0], bd),
              cc.ratio(gx, (gp[..., 0] + 1j * gp[..., 1])[0, 0], bx))
    print('%s: error / bound  W %.3f  gdata %.3f  gparams %.3f' % ((tag,) + ratios))
    assert max(ratios) <= 1.0
    assert np.abs(W).max() > 0.1 and np.abs(gd).max() > 0.1 and np.abs(gx).max() > 0.1


def test_recorded_cases_cover_every_keyword():
    kws = [cc.GOLDEN_CASES[t] for t in RECORDED]
    assert {k['prod'] for k in kws} == {'both', 'left', 'right'}
    for key in ('add_I', 'double', 'tb'):
        assert {k[key] for k in kws} == {True, False}, key


def test_setup_coupling_reproduces_the_recorded_attributes(f64):
    g = cc.golden()
    m, bls = golden_module()
    m.setup_coupling()
    for k in ('flat_data_idx', 'flat_conj_idx', 'flat_unconj_idx', 'flat_data_null', 'bls_idx'):
        assert np.array_equal(getattr(m, k).numpy(), g[k]), k
    assert np.array_equal(m.I.numpy(), g['I']) and m.I.shape == (1, 1, 8, 8, 1, 1)
    for tag, kw in (('ct', dict(conj=True)), ('cf', dict(conj=False)), ('ct_min', dict(conj=True, min_dly=20.0)),
                    ('cf_min', dict(conj=False, min_dly=20.0))):
        m.setup_coupling(**kw)
        assert m.dly.shape == (1, 1, 8, 8, 1, cc.NF)
        # two float64 evaluations of the phasor: coupling_common.dly_ulps (derived from the largest phase, ~100 rad)
        assert np.abs(m.dly.numpy() - g['dly_' + tag]).max() <= cc.dly_ulps(g['freqs'], g['antvecs']) * cc.U['f64'], tag
    # the table against the restatement's own loops, and the null entries
    table, out_rows = cc.build_table([int(a) for a in g['ants']], bls)
    assert np.array_equal(m.plan.table, table) and np.array_equal(m.plan.out_rows, out_rows)
    assert (table == -1).sum() == 2 * 2 + 1 and m.plan.Nbl == len(bls) == 33 and not m.plan.unread
    assert [int(a) for a in g['ants']] != sorted(int(a) for a in g['ants'])


def test_setup_coupling_refuses_what_the_reference_mangles():
    m, bls = golden_module()
    a, b = bls[0] if bls[0][0] != bls[0][1] else bls[1]
    with pytest.raises(ValueError, match='ant2 >= ant1'):
        m.setup_coupling(bls=[(b, a)] + bls[2:])
    with pytest.raises(ValueError, match='twice'):
        m.setup_coupling(bls=bls + [bls[3]])
    with pytest.raises(ValueError, match='not in antpos'):
        m.setup_coupling(bls=bls + [(a, 999)])
    m.setup_coupling(bls=bls)


def test_plan_tables_on_crafted_inputs():
    from bayeslim_amd import ops
    C = ops.COUPLING_CONJ
    table = np.array([[0, 1, -1], [1 | C, -1, 2], [-1, 2 | C, 3]])
    plan = ops.CouplingPlan(table, [1, 0, 8], 5)
    assert plan.N == 3 and plan.Nbl == 5 and plan.Nout == 3 and plan.unread           # row 4 is outside the matrix
    assert np.array_equal(plan.otab, [[1, 0, -1], [-1, -1, -1], [-1, -1, 2]])
    assert np.array_equal(plan.ftab, [[0 | C, 1, -1], [-1, -1, 2], [-1, -1, 3 | C]])  # autos: the single term
    assert plan.table.dtype == plan.otab.dtype == plan.ftab.dtype == np.int32
    pickle.loads(pickle.dumps(plan))
    for bad, rows, Nbl in ((np.zeros((2, 3), int), [0], 1), (np.array([[5]]), [0], 5), (np.array([[-2]]), [0], 1),
                           (np.array([[0, 0], [-1, -1]]), [0], 1), (np.array([[-1, 0 | C], [-1, -1]]), [0], 1),
                           (np.array([[0]]), [1], 1), (np.array([[0, -1], [-1, -1]]), [0, 0], 1),
                           (np.array([[0.5]]), [0], 1), (np.array([[0]]), [], 1), (np.array([[4 * C]]), [0], 1),
                           # row 0 plain at (0, 1) but conjugated at (2, 0), not at the transposed entry: the fold cannot express it
                           (np.array([[-1, 0, -1], [-1, -1, -1], [0 | C, -1, -1]]), [1], 1)):
        with pytest.raises(ValueError):
            ops.CouplingPlan(bad, rows, Nbl)


def test_entry_points_reject_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)                          # non-null dummy; never dereferenced on a rejected call
    big = 1 << 40

    def fwd(dtype=0, x=one, data=one, tab=one, otab=one, out=one, N=4, Nbl=10, Nout=10, Nt=3, Nf=5, Tm=3, Fm=5, addI=1, prod=0,
            ws=one, nbytes=big):
        return lib.rime_coupling_fwd(dtype, x, None, data, tab, otab, N, Nbl, Nout, Nt, Nf, Tm, Fm, addI, prod, out, ws, nbytes, None)

    def bwd(dtype=0, x=one, data=one, gout=one, tab=one, otab=one, ftab=one, N=4, Nbl=10, Nout=10, Nt=3, Nf=5, Tm=1, Fm=5, addI=1,
            prod=0, gdata=one, gx=one, ws=one, nbytes=big):
        return lib.rime_coupling_bwd(dtype, x, None, data, gout, tab, otab, ftab, N, Nbl, Nout, Nt, Nf, Tm, Fm, addI, prod,
                                     gdata, gx, ws, nbytes, None)

    for k in ('x', 'data', 'tab', 'otab', 'out'):
        assert fwd(**{k: None}) == -1, k
    for kw in (dict(N=0), dict(Nt=0), dict(Nf=0), dict(Nbl=0), dict(Nout=0), dict(Tm=2), dict(Fm=4), dict(Fm=0), dict(dtype=2),
               dict(prod=3), dict(prod=-1), dict(addI=2)):
        assert fwd(**kw) == -1, kw
    need = lib.rime_coupling_workspace(0, 4, 3, 5, 3, 5, 0, 0)
    assert need == 4 * 4 * 3 * 5 * 8
    assert fwd(ws=None) == -2 and fwd(nbytes=need - 1) == -2
    assert fwd(prod=1, ws=None, Fm=4) == -1           # a one-sided product needs no workspace, but the shape is still checked
    for k in ('x', 'data', 'gout', 'tab', 'otab', 'ftab'):
        assert bwd(**{k: None}) == -1, k
    assert bwd(gdata=None, gx=None) == -1
    for kw in (dict(N=0), dict(Tm=2), dict(Fm=3), dict(dtype=-1), dict(prod=5), dict(addI=-1)):
        assert bwd(**kw) == -1, kw
    assert bwd(ws=None) == -2 and bwd(nbytes=lib.rime_coupling_workspace(0, 4, 3, 5, 1, 5, 0, 1) - 1) == -2
    assert bwd(prod=1, Tm=3, ws=None, nbytes=0, N=0) == -1
    assert lib.rime_coupling_expand(0, None, None, 4, 3, 5, 3, 5, 1, one, None) == -1
    assert lib.rime_coupling_expand(0, one, None, 4, 3, 5, 2, 5, 1, one, None) == -1
    assert lib.rime_coupling_expand(3, one, None, 4, 3, 5, 3, 5, 1, one, None) == -1
    assert lib.rime_coupling_expand_bwd(0, one, None, None, 4, 3, 5, 3, 5, one, None, 0, None) == -1
    assert lib.rime_coupling_expand_bwd(0, one, None, one, 4, 3, 5, 3, 1, one, None, 0, None) == -2      # f broadcast: workspace


def test_workspace_query():
    from bayeslim_amd._lib import lib
    ws = lib.rime_coupling_workspace
    mat = 128 * 128 * 8 * 256 * 8                     # one (N, N, Nt, Nf) complex64 matrix of HERA-128, 8 times, 256 channels
    assert ws(0, 128, 8, 256, 8, 256, 0, 0) == mat and ws(0, 128, 8, 256, 8, 256, 1, 0) == 0 == ws(0, 128, 8, 256, 8, 256, 2, 0)
    assert ws(0, 128, 8, 256, 8, 256, 0, 1) == 2 * mat and ws(0, 128, 8, 256, 1, 256, 0, 1) == 3 * mat
    assert ws(0, 128, 8, 256, 1, 256, 1, 1) == mat and ws(0, 128, 8, 256, 8, 256, 2, 1) == 0
    assert ws(0, 128, 8, 256, 8, 256, 0, 2) == 0 and ws(0, 128, 8, 256, 8, 1, 0, 2) == mat
    small = 33 * 33 * 3 * 37 * 16                     # complex128
    assert ws(1, 33, 3, 37, 3, 37, 0, 0) == small and ws(1, 33, 3, 37, 3, 1, 0, 1) == 3 * small
    assert ws(0, 0, 3, 37, 3, 37, 0, 0) == 0 and ws(0, 33, 3, 37, 2, 37, 0, 0) == 0 and ws(0, 33, 3, 37, 3, 37, 0, 3) == 0


def test_module_bookkeeping_without_a_gpu():
    from bayeslim_amd import calibration, dataset
    g = cc.golden()
    m, bls = golden_module(add_I=False, prod='left', double=True, name='coupling')
    assert m.name == 'coupling' and (m.add_I, m.prod, m.double) == (False, 'left', True)
    assert isinstance(m.params, torch.nn.Parameter) and m.named_params == ['params']
    assert m.Nants == 8 and m.Nfreqs == cc.NF and m.Npol == 1 and m._vd is None
    vd = dataset.VisData()
    vd.setup_data(bls, g['times'], g['freqs'], pol='ee', data=torch.as_tensor(g['data']))
    with pytest.raises(RuntimeError, match='setup_coupling'):
        m(vd)
    m.setup_coupling()
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        m(vd)
    # one time bin broadcasts, several are indexed through the time cache
    x = torch.zeros(1, 1, 8, 8, 1, cc.NF)
    assert m.index_params(x, times=vd.times[:2]) is x
    y = torch.arange(cc.NT, dtype=torch.float64)[:, None].expand(1, 1, 8, 8, cc.NT, cc.NF)
    assert torch.equal(m.index_params(y, times=vd.times[1:])[0, 0, 0, 0, :, 0], torch.tensor([1.0, 2.0]))
    assert len(m.cache_tidx) == 1
    m.clear_cache()
    assert m.cache_tidx == {} and m._vd is None
    m.push(torch.float32)
    assert m.params.dtype == torch.float32 and m.dly.dtype == torch.complex64 and m.I.dtype == torch.float32
    assert isinstance(m.params, torch.nn.Parameter) and m.flat_data_idx.dtype == torch.int64
    m2 = pickle.loads(pickle.dumps(m))
    m3 = copy.deepcopy(m)
    for other in (m2, m3):
        assert np.array_equal(other.plan.table, m.plan.table) and torch.equal(other.dly, m.dly)
    with pytest.raises(AssertionError, match='multi-pol'):
        calibration.VisCoupling(torch.zeros(2, 2, 8, 8, 1, 1, 2), m.freqs, m.antpos, bls)
    assert 'RedVisCoupling' in calibration.VisCoupling.__doc__ and 'gen_coupling_terms' in calibration.VisCoupling.__doc__


def test_ops_refuse_cpu_tensors():
    from bayeslim_amd import ops
    plan = ops.CouplingPlan(np.array([[0]]), [0], 1)
    x = torch.zeros(1, 1, 1, 1, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ops.coupling_apply(x, None, torch.zeros(1, 1, 1, dtype=torch.complex64), plan)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ops.coupling_expand(x)
