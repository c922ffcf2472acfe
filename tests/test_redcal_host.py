"""
CPU-side checks of redundant calibration (bayeslim_amd/calibration.py, ops.RedVisPlan, rime_redvis_fwd / rime_redvis_bwd):
the plan tables on crafted inputs, the degeneracy tools and the JonesResponse projection on CPU tensors against the
reference's recorded results (tests/golden/redcal.npz, float64, rtol 1e-10), vis2RedVisModel / vis2JonesModel, the refusal
of CPU tensors, argument validation of the two entry points without a GPU, and the no-scratch property of the built kernels.
"""
import ctypes
import pickle
import re

import numpy as np
import pytest
import torch

import redcal_common as rc
import kernel_asm

RTOL = 1e-10


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def close(a, b, tol=RTOL):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape and a.is_complex() == b.is_complex(), (a.shape, b.shape, a.dtype, b.dtype)
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


def setup():
    from bayeslim_amd import utils
    g = {k: torch.as_tensor(v) for k, v in rc.golden().items()}
    ants = [int(a) for a in g['ants']]
    antpos = utils.AntposDict(ants, g['antvecs'])
    bls = [tuple(int(x) for x in b) for b in g['bls']]
    return g, ants, antpos, bls


def visdata(g, antpos, bls, data=None):
    from bayeslim_amd import dataset
    vd = dataset.VisData()
    vd.setup_meta(None, antpos)
    vd.setup_data(bls, g['times'], g['freqs'], pol='ee', data=g['vis'] if data is None else data)
    return vd


def test_plan_tables_on_crafted_inputs():
    from bayeslim_amd import ops
    red = [2, 0, 2, 5, 0, 2, 3]                                   # groups 1 and 4 empty
    plan = ops.RedVisPlan(red, 6, tmap=[2, 0, 3, 0], Ntm=5)      # model times 1 and 4 unused, 0 used twice
    assert (plan.Nbl, plan.Nred, plan.Nt, plan.Ntm, plan.max_members, plan.identity_t) == (7, 6, 4, 5, 3, False)
    assert plan.goff.tolist() == [0, 2, 2, 5, 6, 6, 7] and plan.gmem.tolist() == [1, 4, 0, 2, 5, 6, 3]
    assert plan.toff.tolist() == [0, 2, 2, 3, 4, 4] and plan.tmem.tolist() == [1, 3, 0, 2]
    for off, mem, idx, N in ((plan.goff, plan.gmem, red, 6), (plan.toff, plan.tmem, plan.tmap, 5)):
        assert sorted(mem.tolist()) == list(range(len(idx)))                             # every entry exactly once
        for r in range(N):
            m = mem[off[r]:off[r + 1]].tolist()
            assert m == sorted(m) and all(idx[i] == r for i in m)                         # in its own list, ascending
        o2, m2 = rc.csr(idx, N)
        assert off.tolist() == o2.tolist() and mem.tolist() == m2.tolist()
    T = plan.tables('cpu')
    assert plan.tables('cpu') is T and all(t.dtype == torch.int32 and t.is_contiguous() for t in T.values())
    assert T['red'].tolist() == red and T['goff'].tolist() == plan.goff.tolist()
    Q = pickle.loads(pickle.dumps(plan))
    assert '_tabs' not in Q.__dict__ and Q.gmem.tolist() == plan.gmem.tolist()
    ident = ops.RedVisPlan(torch.as_tensor(red), 6, Ntm=3)
    assert ident.identity_t and ident.Nt == 3 and ident.toff.tolist() == [0, 1, 2, 3] and ident.tmem.tolist() == [0, 1, 2]
    for bad in (dict(red=[0, 6], Nred=6, Ntm=2), dict(red=[0, -1], Nred=6, Ntm=2), dict(red=[0, 1], Nred=2, tmap=[0, 2], Ntm=2),
                dict(red=[0, 1], Nred=2, tmap=[-1], Ntm=2), dict(red=[0, 1], Nred=2), dict(red=[], Nred=2, Ntm=2),
                dict(red=[0.5], Nred=2, Ntm=2)):
        with pytest.raises(ValueError):
            ops.RedVisPlan(bad.pop('red'), bad.pop('Nred'), **bad)


def test_tuple_and_blnum_keys_give_the_same_plan(f64):
    from bayeslim_amd import calibration as cal, telescope_model, utils
    g, ants, antpos, bls = setup()
    reds, _, bl2red = telescope_model.build_reds(antpos, bls=bls)[:3]
    assert len(reds) == int(g['Nred']) and [bl2red[b] for b in bls] == g['red'].tolist()          # the reference's grouping
    by_num = {utils.ants2blnum(b): r for b, r in bl2red.items()}
    blnums = torch.as_tensor(utils.ants2blnum(bls))
    p = torch.zeros(1, 1, len(reds), 3, 5, 2)
    i1 = cal.RedVisModel(p, bl2red).get_bl_idx(blnums)
    i2 = cal.RedVisModel(p, by_num).get_bl_idx(blnums)
    assert torch.equal(i1, i2) and i1.tolist() == g['red'].tolist()
    with pytest.raises(KeyError):
        cal.RedVisModel(p, {}).get_bl_idx(blnums)


@pytest.mark.parametrize('tag', ['u', 'w'])
def test_degeneracies_of_gains_against_the_reference(f64, tag):
    from bayeslim_amd import calibration as cal
    g, ants, antpos, bls = setup()
    w = None if tag == 'u' else g['wgts_ant']
    a, s = cal.compute_redcal_degen(g['gains'], ants, antpos, wgts=w)
    assert a.shape == (1, 1, 1, 3, 5) and s.shape == (1, 1, 2, 3, 5)
    assert close(a, g['degen_amp_' + tag]) and close(s, g['degen_phs_' + tag])
    assert cal.compute_redcal_degen(g['gains'], ants, antpos, wgts=w, abs_amp=False)[0] is None
    assert cal.compute_redcal_degen(g['gains'], ants, antpos, wgts=w, phs_slope=False)[1] is None
    dg = cal.redcal_degen_gains(abs_amp=a, phs_slope=s, ants=ants, antpos=antpos)
    assert close(dg, g['degen_gains_' + tag]) and close(cal.redcal_degen_gains(abs_amp=a, phs_slope=s, antpos=antpos), dg)
    ng, nv, dgr = cal.remove_redcal_degen(g['gains'], ants, antpos, wgts=w)
    assert nv is None and close(ng, g['rm_gains_' + tag]) and close(dgr, g['rm_degen_' + tag])
    # what is left has no degenerate part: zero amplitude and slope parameters
    a2, s2 = cal.compute_redcal_degen(ng, ants, antpos, wgts=w)
    assert float(a2.abs().max()) < 1e-10 and float(s2.abs().max()) < 1e-10


def test_degeneracy_options_and_visibilities_against_the_reference(f64):
    from bayeslim_amd import calibration as cal
    g, ants, antpos, bls = setup()
    assert close(cal.redcal_degen_gains(abs_amp=g['degen_amp_u']), g['degen_gains_amp_only'])
    ng, _, dg = cal.remove_redcal_degen(g['gains'], ants, antpos, degen=g['new_degen'])
    assert close(ng, g['rm_gains_nd']) and close(dg, g['rm_degen_nd'])
    cbls = [bls[i] for i in g['cross'].tolist()]
    a, s = cal.compute_redcal_degen_vis(g['dvis'], bls=cbls, antpos=antpos)
    assert close(a, g['dvis_amp']) and close(s, g['dvis_phs'])
    vd = visdata(g, antpos, cbls, data=g['dvis'])
    a2, s2 = cal.compute_redcal_degen_vis(vd)
    assert torch.equal(a2, a) and torch.equal(s2, s)
    assert close(cal.redcal_degen_vis(abs_amp=g['dvis_amp1_in']), g['dvis_amp1'])
    both = cal.redcal_degen_vis(abs_amp=a, phs_slope=s, bls=cbls, antpos=antpos)
    assert close(both, g['dvis_both'])
    out = cal.redcal_degen_vis(abs_amp=a, phs_slope=s, vd=vd)
    assert torch.equal(out.data, both) and out.bls == cbls and torch.equal(out.times, vd.times)
    assert cal.redcal_degen_vis() is None and float(cal.redcal_degen_vis(vd=vd).data.abs().max()) == 0
    # weighted: W = diag(w / sum w); uniform weights reproduce the unweighted fit, and the weighted fit solves its normal equations
    w = torch.as_tensor(np.random.default_rng(5).uniform(0.5, 2.0, len(cbls)))
    au, su = cal.compute_redcal_degen_vis(g['dvis'], wgts=torch.full((len(cbls),), 3.0), bls=cbls, antpos=antpos)
    assert close(au, torch.log(torch.exp(a) / len(cbls))) and close(su, s)
    aw, sw = cal.compute_redcal_degen_vis(g['dvis'], wgts=w, bls=cbls, antpos=antpos)
    A = (antpos[[b[0] for b in cbls]] - antpos[[b[1] for b in cbls]])[:, :2]
    resid = torch.angle(g['dvis']) - torch.einsum('ba,ijalm->ijblm', A, sw)
    assert float(torch.einsum('ba,b,ijblm->ijalm', A, w, resid).abs().max()) < 1e-9
    assert close(aw, torch.log((g['dvis'].abs() * w[:, None, None]).sum(2, keepdim=True) / w.sum()))
    # removing the degeneracies of these visibilities leaves none
    a3, s3 = cal.compute_redcal_degen_vis(g['dvis'] / both * len(cbls), bls=cbls, antpos=antpos)
    assert float(s3.abs().max()) < 1e-10


@pytest.mark.parametrize('tag', ['both', 'amp', 'phs_w', 'both_ref'])
def test_jones_response_projection_against_the_reference(f64, tag):
    from bayeslim_amd import calibration as cal
    g, ants, antpos, bls = setup()
    kw = dict(both=dict(abs_amp_gain=True, phs_slope_gain=True), amp=dict(abs_amp_gain=True),
              phs_w=dict(phs_slope_gain=True, wgts_gain=g['wgts_ant']),
              both_ref=dict(abs_amp_gain=True, phs_slope_gain=True, refant_idx=2))[tag]
    R = cal.JonesResponse(param_type='com', antpos=antpos)
    R.setup_projection(**kw)
    p = g['proj_p'].clone().requires_grad_(True)
    y = R(p)
    (y * g['proj_cot_' + tag].conj()).real.sum().backward()
    assert close(y.detach(), g['proj_out_' + tag]) and close(p.grad, g['proj_g_' + tag])
    with pytest.raises(AssertionError, match='antpos'):
        cal.BaseResponse().setup_projection(phs_slope_gain=True)
    plain = cal.JonesResponse(param_type='com')
    assert not plain._projection and torch.equal(plain(g['proj_p']), torch.view_as_complex(g['proj_p']))


def test_vanilla_models_from_a_visdata(f64):
    from bayeslim_amd import calibration as cal, linear_model as lm
    g, ants, antpos, bls = setup()
    vd = visdata(g, antpos, bls)
    rv = cal.vis2RedVisModel(vd)
    assert isinstance(rv, cal.RedVisModel) and tuple(rv.params.shape) == (1, 1, int(g['Nred']), 3, 5, 2)
    assert float(rv.params.detach().abs().max()) == 0 and rv.R.param_type == 'com' and [rv.bl2red[b] for b in bls] == g['red'].tolist()
    assert tuple(cal.vis2RedVisModel(vd, param_type='real').params.shape) == (1, 1, int(g['Nred']), 3, 5)
    jm = cal.vis2JonesModel(vd, refant=3)
    assert isinstance(jm, cal.JonesModel) and tuple(jm.params.shape) == (1, 1, 7, 3, 5, 2) and jm.ants == ants
    assert torch.equal(torch.view_as_complex(jm.params.detach()), torch.ones(1, 1, 7, 3, 5, dtype=torch.complex128))
    assert jm.refant == 3 and jm.polmode == '1pol' and jm.R.antpos is antpos
    assert tuple(cal.vis2JonesModel(vd, param_type='phs').params.shape) == (1, 1, 7, 3, 5)
    assert tuple(cal.vis2JonesModel(vd, param_type='phs_slope').params.shape) == (1, 1, 2, 3, 5)
    assert tuple(cal.vis2JonesModel(vd, single_ant=True).params.shape) == (1, 1, 1, 3, 5, 2)
    # linear mode: the sizes come from the LinearModel
    fLM = lm.LinearModel('poly', dim=-1, x=g['freqs'], Ndeg=2, basis='legendre')
    tLM = lm.LinearModel('poly', dim=-2, x=g['times'] - g['times'][0], Ndeg=2, basis='direct')
    jl = cal.vis2JonesModel(vd, param_type='amp', freq_mode='linear', freq_LM=fLM)
    assert tuple(jl.params.shape) == (1, 1, 7, 3, 2) and jl.R.freq_mode == 'linear'
    rl = cal.vis2RedVisModel(vd, freq_mode='linear', freq_LM=fLM, time_mode='linear', time_LM=tLM)
    assert tuple(rl.params.shape) == (1, 1, int(g['Nred']), 2, 2, 2)


def test_models_refuse_cpu_tensors(f64):
    from bayeslim_amd import calibration as cal, ops
    g, ants, antpos, bls = setup()
    vd = visdata(g, antpos, bls)
    rv = cal.vis2RedVisModel(vd)
    with pytest.raises(RuntimeError, match='needs tensors on the GPU'):
        rv(vd)
    with pytest.raises(RuntimeError, match='needs tensors on the GPU'):
        cal.VisModel(torch.zeros(1, 1, 28, 3, 5))(vd)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ops.redvis(g['vis'], torch.zeros(1, 1, 28, 3, 5, dtype=torch.complex128), ops.RedVisPlan(np.arange(28), 28, Ntm=3))
    with pytest.raises(RuntimeError, match='needs tensors on the GPU'):
        cal.remove_redcal_degen(g['gains'], ants, antpos, redvis=g['rm_redvis'], bls=[bls[i] for i in g['cross'].tolist()])
    assert cal.VisModelResponse().param_type == 'real' and isinstance(rv.R, cal.VisModelResponse)


def test_entry_points_reject_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)      # non-null dummy; never dereferenced on a rejected call

    def fwd(dtype=0, NP=1, vis=one, model=one, red=one, tmap=one, Nbl=4, Nt=3, Nf=5, Nred=2, Ntm=3, st=(30, 15, 5, 1), sign=1, out=one):
        return lib.rime_redvis_fwd(dtype, NP, vis, model, red, tmap, Nbl, Nt, Nf, Nred, Ntm, *st, sign, out, None)

    def bwd(dtype=0, NP=1, gout=one, goff=one, gmem=one, toff=one, tmem=one, Nbl=4, Nt=3, Nf=5, Nred=2, Ntm=3, sign=1, gm=one):
        return lib.rime_redvis_bwd(dtype, NP, gout, goff, gmem, toff, tmem, Nbl, Nt, Nf, Nred, Ntm, sign, gm, None)

    assert fwd(model=None) == -1 and fwd(red=None) == -1 and fwd(out=None) == -1                      # null pointers
    assert fwd(NP=3) == -1 and fwd(NP=0) == -1 and fwd(dtype=2) == -1 and fwd(dtype=-1) == -1
    for k in ('Nbl', 'Nt', 'Nf', 'Nred', 'Ntm'):
        assert fwd(**{k: 0}) == -1 and fwd(**{k: -2}) == -1 and bwd(**{k: 0}) == -1 and bwd(**{k: -2}) == -1, k
    assert fwd(sign=0) == -1 and fwd(sign=2) == -1 and bwd(sign=0) == -1
    assert fwd(st=(30, -15, 5, 1)) == -1 and fwd(st=(-1, 15, 5, 1)) == -1                             # negative strides
    assert fwd(tmap=None, Ntm=4) == -1                                                                # identity needs Ntm == Nt
    for k in ('gout', 'goff', 'gmem', 'toff', 'tmem', 'gm'):
        assert bwd(**{k: None}) == -1, k
    assert bwd(NP=3) == -1 and bwd(dtype=5) == -1


def test_redvis_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/redvis.hip: 4 forward (precision x Npol) and 2 backward kernels, no private
    segment in any"""
    asm, kernels, sizes = kernel_asm.read('redvis')
    assert len(kernels) == 6 and all('redvis_' in k for k in kernels), kernels
    assert len(sizes) == 6 and max(sizes) == 0, sizes
    assert not re.findall(r'global_atomic|flat_atomic', asm)
