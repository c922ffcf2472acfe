"""
GPU checks of the redundant mutual-coupling term: ops.redcoupling_apply (forward and both gradients) against the float64
restatement of tests/redcoupling_common.py within its derived bound for the cases of redcoupling_common.KERNEL_CASES in
complex64 and complex128 (a single baseline, the 7-hexagon with outrigger, a 19-antenna hexagon whose term lists straddle the
segment length; a column nothing reads, terms without an entry, second-order entries with a == b, auto-correlation inputs),
calibration.RedVisCoupling against the reference's recorded results (tests/golden/redcoupling.npz) and against the reference's
analytic check (VisCoupling on the inflated parameters and data; V + X V + V X^H without the second order), bit-identical
gradients, gradcheck, and the chain Sequential(RedVisModel -> RedVisCoupling -> JonesModel) in optim.LogProb.
"""
import numpy as np
import pytest
import torch

import coupling_common as cc
import redcoupling_common as rc
from test_redcoupling_host import fixture_array, golden_bounds, golden_module

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
_ref = {}


def reference(name):
    """entry list, inputs, float64 results, bound moduli and rounding counts of a kernel case, computed once and shared"""
    if name in _ref:
        return _ref[name]
    from bayeslim_amd import calibration as cal
    ants, vecs, bls_in, bls_out, c = rc.case_setup(name)
    antpos = {a: torch.as_tensor(v) for a, v in zip(ants, vecs)}
    terms, idx = cal.gen_coupling_terms(antpos, compress_to_red=c['compress'])
    m = cal.RedVisCoupling(torch.zeros(1, 1, len(terms), 1, 1, 2), torch.linspace(120e6, 180e6, c['Nf']), antpos, terms, bls_in,
                           bls_out, coupling_idx=idx)
    m.setup_coupling(use_reds=c['use_reds'], include_second_order=c['second'], **c.get('setup', {}))
    ent = rc.entries({k: [x.numpy() for x in getattr(m, k)] for k in rc.TUPLES}, len(bls_out), m.red_bl_inds if c['use_reds'] else None)
    Nin, Nout, Nterms = len(bls_in) + ('col' in c.get('extra', ())), len(bls_out), len(terms) + ('term' in c.get('extra', ()))
    c.update(module_plan=m.plan, bls_in=bls_in)
    if c.get('straddle'):
        ent, c['picked'] = rc.straddle(ent, m.plan.term_counts, Nterms)
    c['P'] = rc.build_plan(*ent, Nout, Nin, Nterms)
    c['X'], c['D'], c['data'], c['G'] = rc.case_arrays(c, ent, Nin, Nout, Nterms)
    c.update(ent=ent, dims=(Nout, Nin, Nterms))
    c['want'] = rc.evaluate(c['X'], c['D'], c['data'], ent, Nout, G=c['G'])
    c['mag'] = rc.magnitudes(c['X'], c['D'], c['data'], ent, Nout, G=c['G'])
    c['n'] = rc.roundings(c['P'], c['Nt'], c['Nf'], c['X'].shape[1], c['X'].shape[2])
    _ref[name] = c
    return c


def run_case(c, prec):
    from bayeslim_amd import ops
    T = lambda a: None if a is None else torch.as_tensor(a, device=DEV).to(CDT[prec])
    X, data = T(c['X']).requires_grad_(True), T(c['data']).requires_grad_(True)
    plan = c.setdefault('plan', ops.RedCouplingPlan(*c['ent'], *c['dims']))
    out = ops.redcoupling_apply(X, T(c['D']), data, plan)
    gX, gd = torch.autograd.grad(out, (X, data), grad_outputs=T(c['G']))
    return tuple(t.detach().cpu().numpy() for t in (out, gd, gX)), (X, data), plan


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('name', sorted(rc.KERNEL_CASES))
def test_kernel_parity(name, prec):
    c = reference(name)
    got, (X, data), plan = run_case(c, prec)
    for k in plan._TABLES:
        assert np.array_equal(getattr(plan, k), c['P'][k]), k
    if not c.get('straddle') and not c.get('extra'):
        assert np.array_equal(plan.ent, c['module_plan'].ent) and np.array_equal(plan.tmem, c['module_plan'].tmem)
    assert got[0].shape == c['G'].shape and got[1].shape == c['data'].shape and got[2].shape == c['X'].shape
    ratios = [rc.ratio(g, w, rc.bound(m, nk, prec, nr)) for g, w, m, nk, nr in zip(got, c['want'], c['mag'], *c['n'])]
    print('%s %s: error / bound  out %.3f  gdata %.3f  gX %.3f' % ((name, prec) + tuple(ratios)))
    assert max(ratios) <= 1.0
    assert all(np.abs(w).max() > 0 for w in c['want'])
    assert np.array_equal(X.detach().cpu().numpy(), c['X'].astype(got[0].dtype))
    assert np.array_equal(data.detach().cpu().numpy(), c['data'].astype(got[0].dtype))
    if 'col' in c.get('extra', ()):
        assert plan.coff[-1] == plan.coff[-2] and not got[1][-1].any(), 'a column nothing reads gets an exact zero gradient'
    if 'term' in c.get('extra', ()) or 'setup' in c:
        empty = plan.term_counts == 0
        assert empty.any() and not got[2][empty].any(), 'a term without an entry gets an exact zero gradient'


def test_case_table_covers_the_paths():
    """what the cases were chosen for, asserted on their plans: lists that straddle the segment length and reach a second
    level of the combine, second-order entries with a == b, auto-correlation inputs, conjugated readers"""
    c = reference('hex19')
    counts = c['P']['term_counts']
    got = [int(counts[t]) for t in c['picked']]
    assert got[0] % rc.SEG == rc.SEG - 1 and got[1] % rc.SEG == 0 and got[2] % rc.SEG == 1 and min(got[:3]) > rc.SEG
    assert got[3] > rc.WAVES * rc.SEG, 'a wave of the combine adds more than one segment sum'
    assert c['module_plan'].term_counts.max() > rc.SEG
    row, col, conj, a, b = c['ent']
    assert ((a == b) & (a >= 0)).any() and conj.any() and ((a >= 0) & (b >= 0)).any()
    assert any(bl[0] == bl[1] for bl in c['bls_in'])
    assert reference('pair')['dims'][:2] == (1, 1)
    assert rc.WAVES * rc.COLS == 256 and reference('hex7_fb')['Nf'] > rc.COLS


def test_backward_is_bit_identical_and_gradcheck():
    c = reference('hex19')
    a, _, _ = run_case(c, 'f32')
    b, _, _ = run_case(c, 'f32')
    assert all(np.array_equal(x.view(np.float32), y.view(np.float32)) for x, y in zip(a, b))
    c = reference('hex7_tfb')
    a, _, _ = run_case(c, 'f64')
    b, _, _ = run_case(c, 'f64')
    assert all(np.array_equal(x.view(np.float64), y.view(np.float64)) for x, y in zip(a, b))
    from bayeslim_amd import ops
    c = reference('pair')
    T = lambda x: torch.as_tensor(x, device=DEV).to(torch.complex128)
    plan = ops.RedCouplingPlan(*c['ent'], *c['dims'])
    X, data, D = T(c['X']).requires_grad_(True), T(c['data']).requires_grad_(True), T(c['D'])
    assert torch.autograd.gradcheck(lambda x, d: ops.redcoupling_apply(x, D, d, plan), (X, data), eps=1e-6, atol=1e-7, rtol=1e-6)


def golden_run(tag, min_dly=True):
    """(module, input VisData, output VisData) of a recorded case on the GPU in float64, the loss backpropagated"""
    from bayeslim_amd import dataset
    g, antpos, bls_out, bls_red = fixture_array()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        m, kw, setup = golden_module(tag, device=DEV)
        m.setup_coupling(min_dly=kw.get('min_dly') if min_dly else None, **setup)
        vd = dataset.VisData()
        vd.setup_meta(None, antpos)
        data = torch.as_tensor(g['data_red' if kw['use_reds'] else 'data_phys'], device=DEV).requires_grad_(True)
        vd.setup_data(bls_red if kw['use_reds'] else bls_out, torch.as_tensor(g['times']), torch.as_tensor(g['freqs']), pol='ee', data=data)
        vout = m(vd)
        ((vout.data.real ** 2 + vout.data.imag ** 2) * torch.as_tensor(g['w'], device=DEV)).sum().backward()
    finally:
        torch.set_default_dtype(old)
    return m, vd, vout


@pytest.mark.parametrize('tag', sorted(rc.GOLDEN_CASES))
def test_module_reproduces_the_reference(tag):
    """the recorded cases through calibration.RedVisCoupling in float64; the module evaluates its own delay phasor and the
    bound propagates its distance from the recorded one"""
    g = rc.golden()
    m, vd, vout = golden_run(tag)
    assert vout.data.shape == g['V_' + tag].shape and vout.data.dtype == torch.complex128
    assert [tuple(b) for b in vout.bls] == [tuple(int(x) for x in b) for b in g['bls_out']]
    _, (bv, bd, bx) = golden_bounds(tag, own_dly=True)
    gp, want = m.params.grad.cpu().numpy(), g['gp_' + tag]
    ratios = (rc.ratio(vout.data.detach().cpu().numpy()[0, 0], g['V_' + tag][0, 0], bv),
              rc.ratio(vd.data.grad.cpu().numpy()[0, 0], g['gd_' + tag][0, 0], bd),
              rc.ratio((gp[..., 0] + 1j * gp[..., 1])[0, 0], (want[..., 0] + 1j * want[..., 1])[0, 0], bx))
    print('%s: error / bound  V %.3f  gdata %.3f  gparams %.3f' % ((tag,) + ratios))
    assert max(ratios) <= 1.0
    again = m(vd)
    assert again is vout and torch.equal(again.data, vout.data)


@pytest.mark.parametrize('second', [True, False])
def test_analytic_check(second):
    """the reference's own check (tests/test_calibration.py:57-209): with all terms and use_reds the output equals
    VisCoupling(CouplingInflate(-vecs)(params)) on the inflated data (second order), or V + X V + V X^H (first order only)"""
    from bayeslim_amd import calibration as cal, dataset
    g, antpos, bls_out, bls_red = fixture_array()
    tag = 'red_cmp_sq_pt'
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        m, kw, setup = golden_module(tag, device=DEV)
        m.setup_coupling(**dict(setup, include_second_order=second))
        times, freqs = torch.as_tensor(g['times']), torch.as_tensor(g['freqs'])
        vd = dataset.VisData()
        vd.setup_meta(None, antpos)
        vd.setup_data(bls_red, times, freqs, pol='ee', data=torch.as_tensor(g['data_red'], device=DEV))
        with torch.no_grad():
            got = m(vd).data[0, 0].cpu().numpy()
            cvecs = torch.stack([antpos[b] - antpos[a] for a, b in m.coupling_terms])
            infl = cal.CouplingInflate(-cvecs, antpos)
            assert not infl.zeros.any()
            X = infl(m.R(m.params))                                                   # (1, 1, N, N, Nt, Nf)
            inflated = vd.data[:, :, torch.as_tensor(m.red_bl_inds, device=DEV)]
            if second:
                vc = cal.VisCoupling(torch.view_as_real(X.resolve_conj()).clone(), freqs.to(DEV), antpos, bls_out, parameter=False,
                                     R=cal.VisModelResponse(param_type='com', times=times, device=DEV))
                vc.setup_coupling()
                vin = dataset.VisData()
                vin.setup_meta(None, antpos)
                vin.setup_data(bls_out, times, freqs, pol='ee', data=inflated.contiguous())
                want = vc(vin).data[0, 0].cpu().numpy()
            else:
                ants = list(antpos)
                N = len(ants)
                pos = torch.stack([antpos[a] for a in ants])
                L = torch.linalg.norm(pos[None] - pos[:, None], dim=-1)
                D = torch.exp(2j * np.pi * (freqs - freqs[0])[None, None, None, :] / m.c * L[:, :, None, None])
                Xd = X[0, 0].cpu() * D
                V = torch.zeros(N, N, len(times), len(freqs), dtype=torch.complex128)
                for r, (a1, a2) in enumerate(bls_out):
                    V[ants.index(a1), ants.index(a2)] = inflated[0, 0, r].cpu()
                    if a1 != a2:                                       # the fixture's autos are complex: read as they are
                        V[ants.index(a2), ants.index(a1)] = inflated[0, 0, r].cpu().conj()
                W = V + torch.einsum('iktf,kjtf->ijtf', Xd, V) + torch.einsum('iktf,jktf->ijtf', V, Xd.conj())
                want = torch.stack([W[ants.index(a1), ants.index(a2)] for a1, a2 in bls_out]).numpy()
    finally:
        torch.set_default_dtype(old)
    p = g['p_' + tag]
    Xn, Dn = (p[..., 0] + 1j * p[..., 1])[0, 0], m.dly[0, 0, :, 0].cpu().numpy()
    ent = (m.plan.row, m.plan.col, m.plan.conj, m.plan.a, m.plan.b)
    Mv, _, _ = rc.magnitudes(Xn, Dn, g['data_red'][0, 0], ent, len(bls_out))
    P = rc.build_plan(*ent, len(bls_out), len(bls_red), len(Xn))
    ulps = cc.dly_ulps(g['freqs'], g['antvecs']) / 2
    (nk, _, _), _ = rc.roundings(P, rc.NT, rc.NF, rc.NT, rc.NF, dly=ulps)
    n_other = cc.roundings(len(antpos), rc.NT, rc.NF, rc.NT, rc.NF, 'both', False, dly=ulps)[0]
    r = rc.ratio(got, want, rc.bound(Mv, nk, 'f64', n_other))
    print('analytic check, second order %s: error / bound %.3f' % (second, r))
    assert r <= 1.0 and np.abs(want).max() > 0


def test_deepcopy_after_backward():
    """hex-7, 2 times, 3 channels: a deep copy taken after forward and backward holds no cached output and computes the same
    bits; the original's cached output is untouched"""
    import calterm_common as ct
    ct.check_deepcopy_after_backward('RedVisCoupling', DEV)


def test_chain_in_logprob():
    """Sequential(RedVisModel -> RedVisCoupling -> JonesModel) in optim.LogProb on the fixture's array: closure() gives a finite
    loss and finite, non-zero gradients of all three parameter tensors; with zero coupling the stage is the inflation, bit for bit"""
    from bayeslim_amd import calibration as cal, dataset, optim, utils
    g, antpos_t, bls_out, bls_red = fixture_array()
    rng = np.random.default_rng(15)
    ants = [int(a) for a in g['ants']]
    antpos = utils.AntposDict(ants, g['antvecs'])
    Nred, Nout, Nant, Nt, Nf = len(bls_red), len(bls_out), len(ants), rc.NT, rc.NF
    cx = lambda *s: torch.as_tensor(rng.normal(size=s) + 1j * rng.normal(size=s))
    times, freqs = torch.as_tensor(g['times']), torch.as_tensor(g['freqs'])

    def vdata(bls, d):
        vd = dataset.VisData()
        vd.setup_meta(None, antpos)
        vd.setup_data(bls, times, freqs, pol='ee', data=d.to(DEV))
        return vd

    terms, idx = cal.gen_coupling_terms(antpos, compress_to_red=True, max_len=31.0)
    rv = cal.RedVisModel(torch.view_as_real(cx(1, 1, Nred, Nt, Nf)).clone().to(DEV), {bl: k for k, bl in enumerate(bls_red)},
                         R=cal.VisModelResponse(param_type='com', device=DEV))
    cp = cal.RedVisCoupling(torch.view_as_real(0.05 * cx(1, 1, len(terms), 1, Nf)).clone().to(DEV), freqs.to(DEV), antpos, terms,
                            bls_red, bls_out, coupling_idx=idx, R=cal.VisModelResponse(param_type='com', device=DEV))
    cp.setup_coupling(min_dly=2.0, second_max_len=16.0)
    jm = cal.JonesModel(torch.view_as_real(torch.exp(0.05 * cx(1, 1, Nant, Nt, Nf))).clone().to(DEV), ants,
                        R=cal.JonesResponse(param_type='com', device=DEV))
    model = utils.Sequential(dict(redvis=rv, coupling=cp, cal=jm))
    prob = optim.LogProb(model, dataset.Dataset([vdata(bls_out, cx(1, 1, Nout, Nt, Nf))]),
                         start_inp=[vdata(bls_red, torch.zeros(1, 1, Nred, Nt, Nf, dtype=torch.complex128))], device=DEV)
    loss = prob.closure()
    assert np.isfinite(float(loss)) and float(loss) > 0
    for mod in (rv, cp, jm):
        assert mod.params.grad is not None and bool(torch.isfinite(mod.params.grad).all())
        assert float(mod.params.grad.abs().max()) > 0
    with torch.no_grad():
        cp.params.zero_()
        vin = vdata(bls_red, cx(1, 1, Nred, Nt, Nf))
        for dt in (torch.complex128, torch.complex64):
            vin.data = vin.data.to(dt)
            assert torch.equal(cp(vin).data, vin.data[:, :, torch.as_tensor(cp.red_bl_inds, device=DEV)])


def test_plan_without_a_term_word():
    """no entry names a term: Nseg = 0, the gradient of the coefficients takes no workspace (null pointer, zero bytes) and no
    segment tables, and is zero; out = data[0] + conj(data[1]) and the gradient of the data are exact (one addition of two
    copies, no product)"""
    from bayeslim_amd import ops
    from bayeslim_amd._lib import lib
    plan = ops.RedCouplingPlan(row=[0, 0], col=[0, 1], conj=[0, 1], a=[-1, -1], b=[-1, -1], Nout=1, Nin=2, Nterms=2)
    assert (plan.Nseg, plan.Nmem) == (0, 0) and lib.rime_redcoupling_workspace(ops.RIME_F64, 0, 3, 5) == 0
    rng = np.random.default_rng(8)
    cx = lambda *s: torch.as_tensor(rng.uniform(-1, 1, size=s) + 1j * rng.uniform(-1, 1, size=s))
    X, d, w = cx(2, 1, 1).to(DEV).requires_grad_(True), cx(2, 3, 5).to(DEV).requires_grad_(True), cx(1, 3, 5).to(DEV)
    out = ops.redcoupling_apply(X, None, d, plan)
    gX, gd = torch.autograd.grad((out * w.conj()).real.sum(), [X, d])
    dr = d.detach().clone().requires_grad_(True)
    out_r = (dr[0] + dr[1].conj())[None]
    gdr, = torch.autograd.grad((out_r * w.conj()).real.sum(), [dr])
    assert torch.equal(out, out_r) and torch.equal(gd, gdr)
    assert gX.shape == X.shape and not bool(gX.any())
