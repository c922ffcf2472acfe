"""
GPU checks of redundant calibration: rime_redvis_fwd / rime_redvis_bwd against the float64 restatement of
tests/redcal_common.py within its derived bound (complex64 and complex128, 1 and 2 pols, the cases of
redcal_common.KERNEL_CASES), exact zeros for empty groups and unused model times, bit-identical backward passes, gradcheck,
RedVisModel / VisModel against the reference's recorded results (tests/golden/redcal.npz), the caches and push, and the
redundant-calibration chain Sequential(RedVisModel -> JonesModel) inside optim.LogProb.

Worst error / bound printed by the kernel tests on an MI355X: forward 0 (one float32 add of two inputs of the 2^-20 grid is
exact), backward 0.004 in complex64 (the group of 301 members), 0 in complex128; model gradients in float32 at most 0.34.
"""
import numpy as np
import pytest
import torch

import redcal_common as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
_ref = {}


def reference(name, NP):
    """inputs and float64 results of a kernel case, computed once and shared (read-only)"""
    key = (name, NP)
    if key not in _ref:
        vis, model, gout, red, Nred, tmap, sign = rc.case_inputs(name, NP)
        Nt = rc.KERNEL_CASES[name]['Nt']
        mfull = np.broadcast_to(model, (model.shape[0], Nred, rc.KERNEL_CASES[name]['Ntm'], model.shape[3]))
        out, fmag = rc.fwd_ref(vis, mfull, red, tmap, sign)
        goff, gmem = rc.csr(red, Nred)
        toff, tmem = rc.csr(np.arange(Nt) if tmap is None else tmap, mfull.shape[2])
        gm, bmag, n = rc.bwd_ref(gout, goff, gmem, toff, tmem, sign)
        for a in (out, fmag, gm, bmag, n):
            a.setflags(write=False)
        _ref[key] = dict(vis=vis, model=model, gout=gout, red=red, Nred=Nred, tmap=tmap, sign=sign, out=out, fmag=fmag, gm=gm,
                         bmag=bmag, n=n)
    return _ref[key]


def run_case(name, NP, prec):
    from bayeslim_amd import ops
    r = reference(name, NP)
    c = rc.KERNEL_CASES[name]
    to5 = lambda a: torch.as_tensor(a, dtype=CDT[prec], device=DEV).reshape((NP, NP) + a.shape[1:])
    vis = None if r['vis'] is None else to5(r['vis'])
    base = to5(r['model']).requires_grad_(True)
    model = base.expand(NP, NP, r['Nred'], c['Ntm'], c['Nf']) if c.get('broadcast_time') else base
    plan = ops.RedVisPlan(r['red'], r['Nred'], tmap=r['tmap'], Ntm=c['Ntm'])
    out = ops.redvis(vis, model, plan, undo=r['sign'] < 0)
    gm, = torch.autograd.grad(out, model, to5(r['gout']))
    P = NP * NP
    flat = lambda t: t.detach().cpu().numpy().reshape((P,) + tuple(t.shape[2:]))
    return flat(out), flat(gm), plan


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('NP', [1, 2])
@pytest.mark.parametrize('name', list(rc.KERNEL_CASES))
def test_kernels_against_the_restatement_within_the_bound(name, NP, prec):
    r = reference(name, NP)
    out, gm, plan = run_case(name, NP, prec)
    assert out.shape == r['out'].shape and gm.shape == r['gm'].shape
    rf = rc.ratio(out, r['out'], rc.fwd_bound(r['fmag'], prec))
    rb = rc.ratio(gm, r['gm'], rc.bwd_bound(r['bmag'], r['n'], prec))
    print('redvis %-12s NP %d %s: worst error / bound  forward %.3f  backward %.3f  (largest group %d)'
          % (name, NP, prec, rf, rb, plan.max_members))
    assert rf <= 1 and rb <= 1, (rf, rb)
    if prec == 'f64':                    # gridded inputs: every sum is exact in float64
        assert np.array_equal(out, r['out']) and np.array_equal(gm, r['gm'])
    if name == 'b_ragged':
        assert plan.max_members == 301 and r["n"].max() == 301 and (r['n'][3] == 0).all() and (r['n'][:, 1] == 0).all()


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_empty_groups_and_unused_model_times_are_written_as_zero(prec):
    """every element of gmodel is written by the kernel: a buffer pre-filled with NaN comes back without one, and exactly 0
    where a group has no member (group 3) or a model time no time (model time 1)"""
    from bayeslim_amd import ops
    from bayeslim_amd._lib import lib
    r = reference('b_ragged', 2)
    c = rc.KERNEL_CASES['b_ragged']
    plan = ops.RedVisPlan(r['red'], r['Nred'], tmap=r['tmap'], Ntm=c['Ntm'])
    T = plan.tables(DEV)
    gout = torch.as_tensor(r['gout'], dtype=CDT[prec], device=DEV).contiguous()
    gm = torch.full((4, r['Nred'], c['Ntm'], c['Nf']), float('nan'), dtype=CDT[prec], device=DEV)
    rc_ = lib.rime_redvis_bwd(0 if prec == 'f32' else 1, 2, ops._ptr(torch.view_as_real(gout)), ops._ptr(T['goff']),
                              ops._ptr(T['gmem']), ops._ptr(T['toff']), ops._ptr(T['tmem']), plan.Nbl, plan.Nt, c['Nf'],
                              plan.Nred, plan.Ntm, 1, ops._ptr(torch.view_as_real(gm)), ops._stream())
    assert rc_ == 0
    g = torch.view_as_real(gm)
    assert not torch.isnan(g).any()
    assert (g[:, 3] == 0).all() and (g[:, :, 1] == 0).all() and (g[:, 0, 0] != 0).any()
    assert rc.ratio(gm.cpu().numpy(), r['gm'], rc.bwd_bound(r['bmag'], r['n'], prec)) <= 1


def test_backward_is_bit_identical_from_run_to_run():
    a = run_case('b_ragged', 2, 'f32')[1]
    b = run_case('b_ragged', 2, 'f32')[1]
    assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))


def test_gradcheck_and_the_gradient_of_vis():
    from bayeslim_amd import ops
    rng = np.random.default_rng(2)
    cx = lambda *s: torch.as_tensor(rng.normal(size=s) + 1j * rng.normal(size=s), device=DEV).requires_grad_(True)
    plan = ops.RedVisPlan([1, 0, 1], 2, tmap=[1, 0], Ntm=2)
    vis, model = cx(1, 1, 3, 2, 3), cx(1, 1, 2, 2, 3)
    assert torch.autograd.gradcheck(lambda v, m: ops.redvis(v, m, plan), (vis, model))
    assert torch.autograd.gradcheck(lambda v, m: ops.redvis(v, m, plan, undo=True), (vis, model))
    assert torch.autograd.gradcheck(lambda m: ops.redvis(None, m, plan), (model,))
    out = ops.redvis(vis, model, plan)
    go = torch.randn_like(out)
    gv, gm = torch.autograd.grad(out, (vis, model), go)
    assert gv.data_ptr() == go.data_ptr()                                  # the gradient of vis is gout itself, no copy
    with pytest.raises(ValueError):
        ops.redvis(vis, cx(1, 1, 3, 2, 3), plan)


# ---------------------------------------------------------------------------------------
# RedVisModel / VisModel against the reference
# ---------------------------------------------------------------------------------------
def build_model(tag, prec, g=None):
    from bayeslim_amd import calibration as cal, dataset, utils
    g = g if g is not None else rc.golden()
    cls, ptype, kw = rc.MODEL_CASES[tag]
    rdt = torch.float64 if prec == 'f64' else torch.float32
    T = lambda a: torch.as_tensor(a, device=DEV).to(CDT[prec] if np.iscomplexobj(a) else rdt)
    ants = [int(a) for a in g['ants']]
    antpos = utils.AntposDict(ants, g['antvecs'])
    bls = [tuple(int(x) for x in b) for b in g['bls']]
    times = torch.as_tensor(g['times'])
    R = cal.VisModelResponse(param_type=ptype, times=times, device=DEV)
    p0 = T(g['p0_' + tag]) if kw.get('p0') else None
    if cls == 'RedVisModel':
        bl2red = {bl: int(r) for bl, r in zip(bls, g['red'])}
        model = cal.RedVisModel(T(g['p_' + tag]), bl2red, R=R, p0=p0)
    else:
        model = cal.VisModel(T(g['p_' + tag]), R=R, p0=p0, blnums=torch.as_tensor(utils.ants2blnum(bls)))
    data = g['vis']
    b, t = bls, times
    if kw.get('bsel'):
        data, b = data[:, :, kw['bsel']], [bls[i] for i in kw['bsel']]
    if kw.get('tsel'):
        data, t = data[:, :, :, kw['tsel']], times[kw['tsel']]
    vd = dataset.VisData()
    vd.setup_meta(None, antpos)
    vd.setup_data(b, t, torch.as_tensor(g['freqs']), pol='ee', data=T(data))
    return model, vd, kw


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('tag', list(rc.MODEL_CASES))
def test_models_against_the_reference(tag, prec):
    g = rc.golden()
    model, vd, kw = build_model(tag, prec)
    vout = model(vd, undo=bool(kw.get('undo')))
    cot = torch.as_tensor(g['cot_' + tag], device=DEV).to(CDT[prec])
    (vout.data * cot.conj()).real.sum().backward()
    out, grad = vout.data.detach().cpu().numpy(), model.params.grad.cpu().numpy()
    want, gwant = g['vout_' + tag], g['g_' + tag]
    assert out.shape == want.shape and grad.shape == gwant.shape
    if prec == 'f64':
        assert np.abs(out - want).max() <= 1e-10 * np.abs(want).max()
        assert np.abs(grad - gwant).max() <= 1e-10 * np.abs(gwant).max()
        return
    # float32, derived from the precision alone.  The model value m reaches the kernel with a relative error c u: the
    # parameters (and p0) rounded to float32 and their sum, 2 u for 'com' (the response is a view); for 'amp_phs'
    # exp(a + i phi) with |a|, |phi| <= 2.5 here: 5 u from the rounded arguments, 3 u for exp / sincos and their product,
    # c = 8.  The input is rounded once (u |vis|) and the kernel adds u (|vis| + |m|):
    #     |out - want| <= (c + 2) u (|vis| + |m|),   |m| <= |vis| + |want|
    # Backward: n cotangents rounded once each and summed by the kernel, (gamma_n + u) n max|cot| per component; 'com' hands
    # that on unchanged; 'amp_phs' multiplies by conj(m) (relative error c u, products 3 u): a factor max|m| = exp(max a) and
    # 2 for the two components of a complex product.  n: the largest group of the grouping, 1 for a per-baseline model.
    u = rc.U['f32']
    cls, ptype, _ = rc.MODEL_CASES[tag]
    c = 8 if ptype == 'amp_phs' else 2
    assert np.abs(out - want).max() <= (c + 2) * u * (2 * np.abs(g['vis']).max() + np.abs(want).max())
    n = int(np.bincount(g['red']).max()) if (cls == 'RedVisModel' and not kw.get('full')) else 1
    mmax = float(np.exp(g['p_' + tag][..., 0].max())) if ptype == 'amp_phs' else 1.0
    fac = 2 * max(mmax, 1.0) if ptype == 'amp_phs' else 1.0
    bound = (rc.gamma(n, u) + u + ((c + 3) * u if ptype == 'amp_phs' else 0)) * n * np.abs(g['cot_' + tag]).max() * fac
    worst = np.abs(grad - gwant).max() / bound
    print('%s f32: gradient error / bound %.3f (n = %d)' % (tag, worst, n))
    assert worst <= 1


def test_vd_cache_and_push_round_trip():
    model, vd, _ = build_model('rv_com', 'f64')
    a = model(vd)
    first = a.data.clone()
    assert model._vd is a and len(model.cache_plan) == 1 and len(model.cache_bidx) == 1
    b = model(vd)
    assert b is a and torch.equal(b.data, first) and len(model.cache_plan) == 1           # cached VisData and plan reused
    model.push(torch.float32)
    assert model.params.dtype == torch.float32 and isinstance(model.params, torch.nn.Parameter)
    vd32 = vd.copy(copydata=True)
    vd32.data = vd32.data.to(torch.complex64)
    assert model(vd32).data.dtype == torch.complex64
    model.push(torch.float64)
    # float64 -> float32 -> float64 rounds the parameters once; the same rounded parameters give the same bits again
    c = model(vd).data.clone()
    model.push(torch.float32)
    model.push(torch.float64)
    assert torch.equal(model(vd).data, c)
    model.push('cpu')
    assert model._vd is None and model.cache_plan == {} and model.params.device.type == 'cpu'
    model.push(DEV)
    assert torch.equal(model(vd).data, c)
    model.clear_cache()
    assert model._vd is None and model.cache_bidx == {} and model.cache_tidx == {}


@pytest.mark.parametrize('name', ['JonesModel', 'RedVisModel'])
def test_deepcopy_after_backward(name):
    """hex-7, 2 times, 3 channels: a deep copy taken after forward and backward holds no cached output (whose data is a node
    of the graph for RedVisModel) and computes the same bits"""
    import calterm_common as ct
    ct.check_deepcopy_after_backward(name, DEV)


def test_remove_redcal_degen_with_redvis_against_the_reference():
    from bayeslim_amd import calibration as cal, utils
    g = rc.golden()
    ants = [int(a) for a in g['ants']]
    antpos = utils.AntposDict(ants, g['antvecs'])
    bls = [tuple(int(x) for x in g['bls'][i]) for i in g['cross']]
    T = lambda a: torch.as_tensor(a, device=DEV)
    ng, nv, dg = cal.remove_redcal_degen(T(g['gains']), ants, antpos, redvis=T(g['rm_redvis']), bls=bls)
    for got, key in ((ng, 'rm_gains_rv'), (nv, 'rm_newvis'), (dg, 'rm_degen_u')):
        assert np.abs(got.cpu().numpy() - g[key]).max() <= 1e-10 * np.abs(g[key]).max(), key


def test_redcal_chain_in_logprob():
    """Sequential(RedVisModel -> JonesModel) in optim.LogProb on hex-7, data g_i g_j^* R_red + noise: the gradient of the loss
    with respect to both parameter tensors against the same chain in float64 torch on the CPU (1e-9 relative), and 20 LBFGS
    iterations lower the loss"""
    from bayeslim_amd import calibration as cal, dataset, optim, utils
    g = rc.golden()
    rng = np.random.default_rng(11)
    ants = [int(a) for a in g['ants']]
    antpos = utils.AntposDict(ants, g['antvecs'])
    keep = [int(i) for i in g['cross']]
    bls = [tuple(int(x) for x in g['bls'][i]) for i in keep]
    groups = sorted(set(int(g['red'][i]) for i in keep))
    red = np.array([groups.index(int(g['red'][i])) for i in keep])
    Nbl, Nred, Nant, Nt, Nf = len(bls), len(groups), len(ants), 3, 5
    cx = lambda *s: torch.as_tensor(rng.normal(size=s) + 1j * rng.normal(size=s))
    gains_true = torch.exp(0.1 * cx(1, 1, Nant, Nt, Nf))
    red_true = cx(1, 1, Nred, Nt, Nf)
    i1, i2 = [ants.index(b[0]) for b in bls], [ants.index(b[1]) for b in bls]
    data = gains_true[:, :, i1] * gains_true[:, :, i2].conj() * red_true[:, :, red] + 0.01 * cx(1, 1, Nbl, Nt, Nf)
    times, freqs = torch.as_tensor(g['times']), torch.as_tensor(g['freqs'])

    def vdata(d):
        vd = dataset.VisData()
        vd.setup_meta(None, antpos)
        vd.setup_data(bls, times, freqs, pol='ee', data=d.to(DEV))
        return vd

    pr = torch.view_as_real(red_true + 0.1 * cx(1, 1, Nred, Nt, Nf)).clone()
    pg = torch.view_as_real(torch.ones(1, 1, Nant, Nt, Nf, dtype=torch.complex128) + 0.02 * cx(1, 1, Nant, Nt, Nf)).clone()
    rv = cal.RedVisModel(pr.clone().to(DEV), {bl: int(r) for bl, r in zip(bls, red)},
                         R=cal.VisModelResponse(param_type='com', device=DEV))
    jm = cal.JonesModel(pg.clone().to(DEV), ants, R=cal.JonesResponse(param_type='com', device=DEV))
    model = utils.Sequential(dict(redvis=rv, cal=jm))
    prob = optim.LogProb(model, dataset.Dataset([vdata(data)]), start_inp=[vdata(torch.zeros_like(data))], device=DEV)
    loss0 = prob.closure()
    # the same chain in float64 on the CPU
    a, b = pr.clone().requires_grad_(True), pg.clone().requires_grad_(True)
    G = torch.view_as_complex(b)
    pred = G[:, :, i1] * G[:, :, i2].conj() * torch.view_as_complex(a)[:, :, red]
    ref = ((pred - data).abs() ** 2).sum()
    ref.backward()
    assert abs(float(loss0) - float(ref)) <= 1e-6 * float(ref)          # LogProb returns the loss through a float32 accumulator
    for got, want in ((rv.params.grad, a.grad), (jm.params.grad, b.grad)):
        assert float((got.cpu() - want).abs().max()) <= 1e-9 * float(want.abs().max())
    opt = torch.optim.LBFGS(prob.parameters(), max_iter=20, line_search_fn='strong_wolfe')
    opt.step(prob.closure)
    with torch.no_grad():
        loss1 = prob()
    print('redcal chain: loss %.4e -> %.4e after 20 LBFGS iterations' % (float(loss0), float(loss1)))
    assert float(loss1) < float(loss0)
