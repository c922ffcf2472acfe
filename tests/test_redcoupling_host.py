"""
CPU-side checks of the redundant mutual-coupling term (calibration.RedVisCoupling, CouplingInflate, gen_coupling_terms,
configure_coupling_matrix_singlepath, cut_bl, ops.RedCouplingPlan, telescope_model.build_reds(red_bls=)): the host functions
and the index tuples against the reference's recorded results (tests/golden/redcoupling.npz, redcoupling_arows.json) exactly,
the plan against the explicit-loop restatement of tests/redcoupling_common.py, the restatement's forward and gradients against
the recorded ones within the derived bound (u = 2^-53), every refusal, argument validation of the entry points without a GPU,
and pickle / deepcopy of a set-up module.
"""
import copy
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch

import coupling_common as cc
import redcoupling_common as rc
from bayeslim_amd import calibration as cal, dataset, ops, telescope_model, utils
from bayeslim_amd._lib import lib

TAGS = sorted(rc.GOLDEN_CASES)


def fixture_array():
    g = rc.golden()
    antpos = {int(a): torch.as_tensor(v) for a, v in zip(g['ants'], g['antvecs'])}
    pairs = lambda x: [tuple(int(y) for y in b) for b in x]
    return g, antpos, pairs(g['bls_out']), pairs(g['bls_red'])


def golden_module(tag, device='cpu'):
    """the module of a recorded case, set up (no GPU needed for that), and its keywords"""
    g, antpos, bls_out, bls_red = fixture_array()
    kw = rc.GOLDEN_CASES[tag]
    terms = [tuple(int(x) for x in t) for t in g['terms_' + tag]]
    idx = {tuple(int(x) for x in k): int(v) for k, v in zip(g['idx_keys_' + tag], g['idx_vals_' + tag])}
    R = cal.VisModelResponse(param_type='com', times=None if kw['tb'] else torch.as_tensor(g['times']), device=device)
    m = cal.RedVisCoupling(torch.as_tensor(g['p_' + tag]).to(device), torch.as_tensor(g['freqs']).to(device), antpos, terms,
                           bls_red if kw['use_reds'] else bls_out, bls_out, coupling_idx=idx, R=R)
    return m, kw, dict(use_reds=kw['use_reds'], include_second_order=kw['second'], **kw.get('setup', {}))


def golden_reference(tag):
    """(X, D, data, w, ent, Nout) of a recorded case from the fixture's own tuples"""
    g = rc.golden()
    kw = rc.GOLDEN_CASES[tag]
    p = g['p_' + tag]
    tuples = {k: [g['%s_%d_%s' % (k, n, tag)] for n in range(5 if k.startswith('sq') else 3)] for k in rc.TUPLES}
    Nout = len(g['bls_out'])
    ent = rc.entries(tuples, Nout, g['red_bl_inds_' + tag] if kw['use_reds'] else None)
    data = g['data_red' if kw['use_reds'] else 'data_phys'][0, 0]
    return (p[..., 0] + 1j * p[..., 1])[0, 0], g['dly_' + tag][0, 0, :, 0], data, g['w'][0, 0], ent, Nout


def golden_bounds(tag, own_dly=False):
    """(V, gdata, gX, their bounds) of the restatement for a recorded case; the cotangent 2 w V comes from the output"""
    g = rc.golden()
    X, D, data, w, ent, Nout = golden_reference(tag)
    V, _, _ = rc.evaluate(X, D, data, ent, Nout)
    _, gd, gx = rc.evaluate(X, D, data, ent, Nout, G=2 * w * V)
    Mv, _, _ = rc.magnitudes(X, D, data, ent, Nout)
    _, Md, Mx = rc.magnitudes(X, D, data, ent, Nout, G=2 * w * Mv)
    P = rc.build_plan(*ent, Nout, data.shape[0], X.shape[0])
    m = cc.dly_ulps(g['freqs'], g['antvecs']) / 2 if own_dly else 0
    _, (nf, nd, nx) = rc.roundings(P, data.shape[1], data.shape[2], X.shape[1], X.shape[2], dly=m)
    return (V, gd, gx), (rc.bound(Mv, nf, 'f64', nf), rc.bound(Md, nd + nf + 2, 'f64', nd + nf + 2),
                         rc.bound(Mx, nx + nf + 2, 'f64', nx + nf + 2))


def test_gen_coupling_terms_and_inflate_reproduce_the_reference():
    g, antpos, bls_out, _ = fixture_array()
    ants = [int(a) for a in g['ants']]
    terms, idx = cal.gen_coupling_terms(antpos, ants=[ants[1], ants[4]], min_len=1.0, max_EW=40.0, max_NS=20.0)
    assert np.array_equal(np.array(terms), g['terms_ants']) and idx == {t: i for i, t in enumerate(terms)}
    for tag, kw in rc.GOLDEN_CASES.items():
        terms, idx = cal.gen_coupling_terms(antpos, compress_to_red=kw['compress'], no_auto_coupling=kw.get('no_auto', False),
                                            max_len=kw.get('term_max_len'))
        assert np.array_equal(np.array(terms), g['terms_' + tag])
        assert [list(k) for k in idx] == g['idx_keys_' + tag].tolist() and list(idx.values()) == g['idx_vals_' + tag].tolist()
    infl = cal.CouplingInflate(torch.as_tensor(g['inflate_vecs']), antpos)
    assert np.array_equal(infl.idx.numpy(), g['inflate_idx']) and np.array_equal(infl.zeros.numpy(), g['inflate_zeros'])
    assert infl.zeros.any() and not infl.zeros.all()
    p = torch.randn(1, 1, len(g['inflate_vecs']), 2, 3, dtype=torch.complex128)
    keep = p.clone()
    E = infl(p)
    assert torch.equal(p, keep) and E.shape == (1, 1, 8, 8, 2, 3)
    flat = E.reshape(1, 1, 64, 2, 3)
    assert torch.equal(flat[:, :, ~infl.zeros], p[:, :, infl.idx[~infl.zeros]]) and not flat[:, :, infl.zeros].any()


def test_cut_bl():
    _, antpos, _, _ = fixture_array()
    a = list(antpos)
    vec = (antpos[a[1]] - antpos[a[0]]).numpy()
    L, ew = float(np.linalg.norm(vec)), abs(float(vec[0]))
    bl = (a[0], a[1])
    assert cal.cut_bl(bl, antpos) is False
    assert cal.cut_bl(bl, antpos, max_len=L - 0.1) and not cal.cut_bl(bl, antpos, max_len=L + 0.1)
    assert cal.cut_bl(bl, antpos, min_len=L + 0.1) and not cal.cut_bl(bl, antpos, min_len=L - 0.1)
    assert cal.cut_bl(bl, antpos, max_EW=ew - 0.1) and not cal.cut_bl(bl, antpos, max_EW=ew + 0.1)
    assert cal.cut_bl(bl, antpos, max_NS=ew - 0.1) and not cal.cut_bl(bl, antpos, max_NS=ew + 0.1)    # the reference's rule
    cache = {}
    cal.cut_bl(bl, antpos, bl_vecs=cache, max_len=1.0)
    assert bl in cache


def test_arows_reproduce_the_reference():
    g, antpos, bls_out, bls_red = fixture_array()
    with open(os.path.join(rc.HERE, 'golden', 'redcoupling_arows.json')) as f:
        want = json.load(f)
    key = lambda bl: '%d_%d' % bl
    for tag, rows in want.items():
        if tag == 'no_auto':
            A = cal.configure_coupling_matrix_singlepath(antpos, bls_out[8:14], no_auto_coupling=True, min_len=1.0, max_EW=30.0,
                                                         second_max_NS=16.0, Nproc=3)
        else:
            kw = rc.GOLDEN_CASES[tag]
            bl2red = None
            if kw['use_reds']:
                reds, _, idx, _, _, _, _ = telescope_model.build_reds(antpos, bls=bls_out, red_bls=bls_red)
                bl2red = {}
                for k in idx:
                    bl2red[k] = reds[idx[k]][0]
                    bl2red[k[::-1]] = reds[idx[k]][0][::-1]
            A = cal.configure_coupling_matrix_singlepath(antpos, bls_out, bl2red=bl2red, include_second_order=kw['second'],
                                                         **kw.get('setup', {}))
        got = {key(bl): {key(k): v for k, v in row.items()} for bl, row in A.items()}
        assert got == want[tag], tag
        assert [list(r) for r in got.values()] == [list(r) for r in want[tag].values()], tag       # key order too
    names = {n for row in want['cuts'].values() for lst in row.values() for n in lst}
    idx = {tuple(int(x) for x in k) for k in g['idx_keys_cuts']}
    pair = lambda n: tuple(int(a) for a in n.split('_')[1:3])
    assert any(pair(t) not in idx for n in names for t in n.split(',')), 'the cuts case must name terms without an index'


def test_build_reds_red_bls():
    _, antpos, bls_out, bls_red = fixture_array()
    base = telescope_model.build_reds(antpos, bls=bls_out)
    order = bls_red[::-1]
    reds, rvec, bl2red, all_bls, lens, angs, tags = telescope_model.build_reds(antpos, bls=bls_out, red_bls=order)
    assert len(reds) == len(order) and all(rb in red for rb, red in zip(order, reds))
    assert sorted(map(tuple, reds)) == sorted(map(tuple, base[0])) and all(bl2red[bl] == i for i, r in enumerate(reds) for bl in r)
    conj = telescope_model.build_reds(antpos, bls=bls_out, red_bls=[bl[::-1] for bl in order] + [(991, 992)])
    assert conj[0] == reds                                         # the conjugate names the group; an unknown one is passed over
    assert len(telescope_model.build_reds(antpos, bls=bls_out, red_bls=order[:3])[0]) == 3


@pytest.mark.parametrize('tag', TAGS)
def test_setup_reproduces_the_reference(tag):
    """index tuples and red_bl_inds exactly, dly within the two-evaluation bound, the hits, and the plan's tables against the
    explicit-loop restatement built from the RECORDED tuples"""
    g = rc.golden()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        m, kw, setup = golden_module(tag)
        m.setup_coupling(**setup)
        dly0 = m.dly.numpy()
        m.setup_coupling(min_dly=kw.get('min_dly'), **setup)
    finally:
        torch.set_default_dtype(old)
    for k in rc.TUPLES:
        t = getattr(m, k)
        assert len(t) == (5 if k.startswith('sq') else 3)
        for n, x in enumerate(t):
            assert x.dtype == torch.int64 and np.array_equal(x.numpy(), g['%s_%d_%s' % (k, n, tag)]), (k, n)
    if kw['use_reds']:
        assert list(m.red_bl_inds) == g['red_bl_inds_' + tag].tolist()
    tol = cc.dly_ulps(g['freqs'], g['antvecs']) * 2.0 ** -53
    for got, want in ((dly0, g['dly0_' + tag]), (m.dly.numpy(), g['dly_' + tag])):
        assert got.shape == want.shape and max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()) <= tol
    assert ('min_dly' in kw) == (not np.array_equal(g['dly0_' + tag], g['dly_' + tag]))
    hits = m.get_coupling_hits()
    assert [hits[t] for t in m.coupling_terms] == g['hits_' + tag].tolist()
    X, D, data, w, ent, Nout = golden_reference(tag)
    P = rc.build_plan(*ent, Nout, data.shape[0], X.shape[0])
    for k in ops.RedCouplingPlan._TABLES:
        assert np.array_equal(getattr(m.plan, k), P[k]) and getattr(m.plan, k).dtype == np.int32, k
    assert (m.plan.Nent, m.plan.Nseg, m.plan.seg) == (P['Nent'], len(P['segterm']), rc.SEG) and rc.SEG == ops.REDCOUPLING_SEG
    if tag == 'cuts':
        assert (m.plan.term_counts == 0).any(), 'the cuts leave terms without an entry'


@pytest.mark.parametrize('tag', TAGS)
def test_restatement_reproduces_the_reference(tag):
    g = rc.golden()
    (V, gd, gx), (bv, bd, bx) = golden_bounds(tag)
    gp = g['gp_' + tag]
    ratios = (rc.ratio(V, g['V_' + tag][0, 0], bv), rc.ratio(gd, g['gd_' + tag][0, 0], bd),
              rc.ratio(gx, (gp[..., 0] + 1j * gp[..., 1])[0, 0], bx))
    print('%s: error / bound  V %.3f  gdata %.3f  gparams %.3f' % ((tag,) + ratios))
    assert max(ratios) <= 1.0


def test_plan_on_crafted_entries():
    """orderings, roles and segments of a small hand-made list: an entry with a == b sits under both roles, a column nothing
    reads and a term without an entry have empty lists, a list of seg + 1 words makes two segments"""
    row, col, conj, a, b = [2, 0, 0, 1, 2], [1, 0, 3, 3, 1], [0, 1, 0, 0, 1], [1, -1, 1, 3, 1], [1, 0, -1, -1, 3]
    plan = ops.RedCouplingPlan(row, col, conj, a, b, Nout=3, Nin=4, Nterms=4, seg=3)
    assert plan.ent.tolist() == [[0, 0 | rc.FLAG, -1, 0], [0, 3, 1, -1], [1, 3, 3, -1], [2, 1, 1, 1], [2, 1 | rc.FLAG, 1, 3]]
    assert plan.roff.tolist() == [0, 2, 3, 5]
    assert plan.coff.tolist() == [0, 1, 3, 3, 5] and plan.cmem.tolist() == [0, 3, 4, 1, 2]
    F = rc.FLAG
    assert plan.toff.tolist() == [0, 1, 5, 5, 7] and plan.tmem.tolist() == [0 | F, 1, 3, 3 | F, 4, 2, 4 | F]
    assert plan.tsoff.tolist() == [0, 1, 3, 3, 4] and plan.segterm.tolist() == [0, 1, 1, 3] and plan.segstart.tolist() == [0, 1, 4, 5]
    assert plan.term_counts.tolist() == [1, 4, 0, 2]
    P = rc.build_plan(row, col, conj, a, b, 3, 4, 4, seg=3)
    assert all(np.array_equal(getattr(plan, k), P[k]) for k in ops.RedCouplingPlan._TABLES)
    plan.__dict__['_tabs'] = {'x': object()}
    again = pickle.loads(pickle.dumps(plan))
    assert '_tabs' not in again.__dict__ and again.tmem.tolist() == plan.tmem.tolist()
    ok = dict(row=[0], col=[0], conj=[0], a=[-1], b=[-1], Nout=1, Nin=1, Nterms=1)
    ops.RedCouplingPlan(**ok)
    for bad in (dict(row=[1]), dict(row=[-1]), dict(col=[1]), dict(col=[-1]), dict(a=[1]), dict(a=[-2]), dict(b=[1]), dict(b=[-2]),
                dict(conj=[2]), dict(row=[]), dict(row=[0, 0]), dict(row=[0.5]), dict(Nterms=0), dict(seg=0)):
        with pytest.raises(ValueError):
            ops.RedCouplingPlan(**{**ok, **bad})


def test_refusals():
    g, antpos, bls_out, bls_red = fixture_array()
    m, kw, setup = golden_module('red_cmp_sq_pt')
    vd = dataset.VisData()
    vd.setup_meta(None, antpos)
    vd.setup_data(bls_red, g['times'], g['freqs'], pol='ee', data=torch.as_tensor(g['data_red']))
    with pytest.raises(RuntimeError, match='setup_coupling'):
        m(vd)
    m.setup_coupling(**setup)
    with pytest.raises(RuntimeError, match='GPU'):
        m(vd)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.redcoupling_apply(torch.zeros(m.Nterms, 1, 1, dtype=torch.complex64), None,
                              torch.zeros(len(bls_red), 3, 5, dtype=torch.complex64), m.plan)
    args = (m.params.detach(), m.freqs, antpos, m.coupling_terms, bls_red)
    for bad in ([(bls_out[9][1], bls_out[9][0])] + bls_out[10:], bls_out + [bls_out[3]], bls_out + [(bls_out[0][0], 977)]):
        with pytest.raises(ValueError):
            cal.RedVisCoupling(*args, bad, coupling_idx=m.coupling_idx).setup_coupling(**setup)
    with pytest.raises(ValueError):
        cal.RedVisCoupling(*args[:4], bls_red, bls_out, coupling_idx=m.coupling_idx).setup_coupling(use_reds=False)


def test_rejected_calls_return_without_a_launch():
    buf = ctypes.create_string_buffer(64)
    one = ctypes.c_void_p(ctypes.addressof(buf))

    def fwd(dtype=0, x=one, dly=None, data=one, ent=one, roff=one, Nout=2, Nin=2, Nterms=2, Nent=3, Nt=3, Nf=5, Tm=3, Fm=5, out=one):
        return lib.rime_redcoupling_fwd(dtype, x, dly, data, ent, roff, Nout, Nin, Nterms, Nent, Nt, Nf, Tm, Fm, out, None)

    def bwd_d(dtype=0, x=one, g=one, ent=one, coff=one, cmem=one, Nout=2, Nin=2, Nterms=2, Nent=3, Nt=3, Nf=5, Tm=1, Fm=1, gd=one):
        return lib.rime_redcoupling_bwd_data(dtype, x, None, g, ent, coff, cmem, Nout, Nin, Nterms, Nent, Nt, Nf, Tm, Fm, gd, None)

    def bwd_c(dtype=1, x=one, data=one, g=one, ent=one, toff=one, tmem=one, st=one, ss=one, tsoff=one, Nout=2, Nin=2, Nterms=2,
              Nent=3, Nmem=4, Nseg=2, seg=64, Nt=3, Nf=5, Tm=3, Fm=1, gx=one, ws=one, nbytes=1 << 20):
        return lib.rime_redcoupling_bwd_coupling(dtype, x, None, data, g, ent, toff, tmem, st, ss, tsoff, Nout, Nin, Nterms, Nent,
                                                 Nmem, Nseg, seg, Nt, Nf, Tm, Fm, gx, ws, nbytes, None)

    for f, ptrs in ((fwd, ('x', 'data', 'ent', 'roff', 'out')), (bwd_d, ('x', 'g', 'ent', 'coff', 'cmem', 'gd')),
                    (bwd_c, ('x', 'data', 'g', 'ent', 'toff', 'tmem', 'st', 'ss', 'tsoff', 'gx'))):
        for p in ptrs:
            assert f(**{p: None}) == -1, (f.__name__, p)
        for bad in (dict(dtype=2), dict(dtype=-1), dict(Nout=0), dict(Nin=0), dict(Nterms=0), dict(Nent=0), dict(Nt=0), dict(Nf=0),
                    dict(Tm=2), dict(Fm=4), dict(Nout=1 << 30), dict(Nent=1 << 30)):
            assert f(**bad) == -1, (f.__name__, bad)
    for bad in (dict(Nmem=-1), dict(Nseg=-1), dict(Nseg=5), dict(Nseg=0), dict(Nmem=0), dict(seg=0), dict(seg=(1 << 20) + 1)):
        assert bwd_c(**bad) == -1, bad
    assert bwd_c(ws=None) == -2 and bwd_c(nbytes=2 * 3 * 5 * 16 - 1) == -2
    assert lib.rime_redcoupling_workspace(1, 2, 3, 5) == 2 * 3 * 5 * 16 and lib.rime_redcoupling_workspace(0, 7, 3, 5) == 7 * 3 * 5 * 8
    assert lib.rime_redcoupling_workspace(2, 2, 3, 5) == 0 and lib.rime_redcoupling_workspace(0, -1, 3, 5) == 0


def test_pickle_and_deepcopy_of_a_set_up_module():
    m, kw, setup = golden_module('cuts')
    m.setup_coupling(min_dly=kw['min_dly'], **setup)
    m.plan.__dict__['_tabs'] = {'cpu': 'stale'}
    m._vd = 'a cached output'
    for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert other._vd is None and '_tabs' not in other.plan.__dict__
        assert torch.equal(other.params, m.params) and torch.equal(other.dly, m.dly)
        assert other.red_bl_inds == m.red_bl_inds and other.coupling_idx == m.coupling_idx
        for k in rc.TUPLES:
            assert all(torch.equal(a, b) for a, b in zip(getattr(other, k), getattr(m, k)))
        assert np.array_equal(other.plan.ent, m.plan.ent) and np.array_equal(other.plan.tmem, m.plan.tmem)
