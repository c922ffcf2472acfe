"""
GPU checks of the mutual-coupling term: ops.coupling_apply (forward and both gradients) against the float64 restatement of
tests/coupling_common.py within its derived bound for the cases of coupling_common.KERNEL_CASES in complex64 and complex128,
calibration.VisCoupling against the reference's recorded results (tests/golden/coupling.npz), the adjoint identity in float64,
bit-identical gradients, output integrity, and the chain Sequential(RedVisModel -> VisCoupling -> JonesModel) in optim.LogProb.

Worst error / bound printed on an MI355X: kernel cases 0.13 in complex64 and 0.09 in complex128 (both at N = 3, where the
bound is smallest), at N = 65 0.002; the module, with its own delay phasor, against the fixture 0.024 of the
bound that propagates the phasor's rounding; the adjoint identity differs by 1e-14 ... 5e-11
against tolerances of 1e-10 ... 4e-5.
"""
import numpy as np
import pytest
import torch

import coupling_common as cc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
_ref = {}


def reference(name):
    """inputs, float64 results, bound moduli and rounding counts of a kernel case, computed once and shared (read-only)"""
    if name not in _ref:
        c = cc.case_inputs(name)
        args = (c['table'], c['out_rows'], c['add_I'], c['prod'], c['double'])
        c['want'] = cc.evaluate(c['X'], c['D'], c['data'], *args, G=c['G'])
        c['mag'] = cc.magnitudes(c['X'], c['D'], c['data'], *args, G=c['G'])
        c['n'] = cc.roundings(c['N'], c['Nt'], c['Nf'], c['X'].shape[2], c['X'].shape[3], c['prod'], c['double'])
        _ref[name] = c
    return _ref[name]


def run_case(c, prec, plan=None):
    """(W, gdata, gX) of ops.coupling_apply as numpy arrays, plus the tensors that went in"""
    from bayeslim_amd import ops
    T = lambda a: None if a is None else torch.as_tensor(a, device=DEV).to(CDT[prec])
    X, data = T(c['X']).requires_grad_(True), T(c['data']).requires_grad_(True)
    D, G = T(c['D']), T(c['G'])
    plan = plan or ops.CouplingPlan(c['table'], c['out_rows'], data.shape[0])
    W = ops.coupling_apply(X, D, data, plan, add_I=c['add_I'], prod=c['prod'], double=c['double'])
    gX, gd = torch.autograd.grad(W, (X, data), grad_outputs=G)
    return tuple(t.detach().cpu().numpy() for t in (W, gd, gX)), (X, D, data)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('name', sorted(cc.KERNEL_CASES))
def test_kernel_parity(name, prec):
    c = reference(name)
    got, (X, D, data) = run_case(c, prec)
    assert got[0].shape == (len(c['bls']), c['Nt'], c['Nf']) and got[1].shape == c['data'].shape and got[2].shape == c['X'].shape
    ratios = [cc.ratio(g, w, cc.bound(m, n, prec)) for g, w, m, n in zip(got, c['want'], c['mag'], c['n'])]
    print('%s %s: error / bound  W %.3f  gdata %.3f  gX %.3f' % ((name, prec) + tuple(ratios)))
    assert max(ratios) <= 1.0
    assert all(np.abs(w).max() > 0 for w in c['want'])
    # the inputs are unchanged by forward and backward
    assert np.array_equal(X.detach().cpu().numpy(), c['X'].astype(got[0].dtype))
    assert np.array_equal(data.detach().cpu().numpy(), c['data'].astype(got[0].dtype))


def golden_setup(tag, dtype=torch.float64):
    from bayeslim_amd import calibration, dataset
    g = cc.golden()
    kw = cc.GOLDEN_CASES[tag]
    ants, bls = [int(a) for a in g['ants']], [tuple(int(x) for x in b) for b in g['bls']]
    antpos = {a: torch.as_tensor(v) for a, v in zip(ants, g['antvecs'])}
    times, freqs = torch.as_tensor(g['times']), torch.as_tensor(g['freqs'])
    p = torch.as_tensor(g['p_tb' if kw['tb'] else 'p_pt'], device=DEV).to(dtype)
    R = calibration.VisModelResponse(param_type='com', times=times if not kw['tb'] else None, device=DEV)
    m = calibration.VisCoupling(p, freqs.to(DEV), antpos, bls, R=R)
    m.setup_coupling()
    vd = dataset.VisData()
    vd.setup_meta(None, antpos)
    data = torch.as_tensor(g['data'], device=DEV).requires_grad_(True)
    vd.setup_data(bls, times, freqs, pol='ee', data=data)
    return m, vd, data, kw


@pytest.mark.parametrize('tag', sorted(k[2:] for k in cc.golden() if k.startswith('W_')))
def test_module_reproduces_the_reference(tag):
    """the recorded cases through calibration.VisCoupling in float64: the reference summed in another order, so both orders
    are counted (coupling_common.golden_bounds: gamma_n(2^-53) for the kernel plus gamma_n(2^-53) for the fixture); the module
    evaluates its own delay phasor, and the bound propagates its distance from the recorded one (own_dly)"""
    g = cc.golden()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        m, vd, data, kw = golden_setup(tag)
        vout = m(vd, add_I=kw['add_I'], prod=kw['prod'], double=kw['double'])
        assert vout.data.shape == g['W_' + tag].shape and vout.data.dtype == torch.complex128
        ((vout.data.real ** 2 + vout.data.imag ** 2) * torch.as_tensor(g['w'], device=DEV)).sum().backward()
    finally:
        torch.set_default_dtype(old)
    _, (bw, bd, bx) = cc.golden_bounds(tag, own_dly=True)
    gp = m.params.grad.cpu().numpy()
    want = g['gp_' + tag]
    ratios = (cc.ratio(vout.data.detach().cpu().numpy()[0, 0], g['W_' + tag][0, 0], bw),
              cc.ratio(data.grad.cpu().numpy()[0, 0], g['gd_' + tag][0, 0], bd),
              cc.ratio((gp[..., 0] + 1j * gp[..., 1])[0, 0], (want[..., 0] + 1j * want[..., 1])[0, 0], bx))
    print('%s: error / bound  W %.3f  gdata %.3f  gparams %.3f' % ((tag,) + ratios))
    assert max(ratios) <= 1.0


@pytest.mark.parametrize('name', ['n8_both', 'n33', 'n3_left', 'n3_right'])
def test_adjoint_identity(name):
    """float64: <G, dW> = <gdata, dV> + <gX, dX> for random directions.  W is linear in the data, so dW along dV is
    W(X, dV) minus the part that does not depend on the data (none: the map is homogeneous); along dX it is the central
    difference (W(X + h dX) - W(X - h dX)) / 2h with h = 2^-8, exact for these single-path cases up to rounding because W
    is at most quadratic in X.  The tolerance is the derived bound of every term: the forward bound of the three outputs
    (two of them divided by 2h) against |G|, and the two gradient bounds against |dV| and |dX|."""
    from bayeslim_amd import ops
    c = reference(name)
    assert not c['double']
    rng = np.random.default_rng(5)
    h = 2.0 ** -8
    dX = rng.normal(size=c['X'].shape) + 1j * rng.normal(size=c['X'].shape)
    dV = rng.normal(size=c['data'].shape) + 1j * rng.normal(size=c['data'].shape)
    (W, gd, gx), _ = run_case(c, 'f64')
    plan = ops.CouplingPlan(c['table'], c['out_rows'], c['data'].shape[0])
    T = lambda a: None if a is None else torch.as_tensor(a, device=DEV)

    def fwd(X, V):
        with torch.no_grad():
            return ops.coupling_apply(T(X), T(c['D']), T(V), plan, add_I=c['add_I'], prod=c['prod']).cpu().numpy()

    dW = fwd(c['X'], dV) + (fwd(c['X'] + h * dX, c['data']) - fwd(c['X'] - h * dX, c['data'])) / (2 * h)
    inner = lambda a, b: float((np.conj(a) * b).real.sum())
    lhs, rhs = inner(c['G'], dW), inner(gd, dV) + inner(gx, dX)
    args = (c['table'], c['out_rows'], c['add_I'], c['prod'], False)
    nf, nd, nx = c['n']
    Mdv = cc.magnitudes(c['X'], c['D'], dV, *args)[0]
    Mh = cc.magnitudes(np.abs(c['X']) + h * np.abs(dX), c['D'], c['data'], *args)[0]
    _, Md, Mx = c['mag']
    absG = np.abs(c['G'])
    tol = 2 * float((absG * (cc.bound(Mdv, nf, 'f64') + 2 * cc.bound(Mh, nf, 'f64') / (2 * h))).sum()) \
        + 2 * float((cc.bound(Md, nd, 'f64') * np.abs(dV)).sum()) + 2 * float((cc.bound(Mx, nx, 'f64') * np.abs(dX)).sum())
    print('%s: <G, dW> %.12e  <g, d> %.12e  difference %.2e  tolerance %.2e' % (name, lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol and abs(lhs) > 1e3 * tol


def test_gradients_are_bit_identical_across_runs():
    c = reference('n65')
    assert (c['N'], c['Nt'], c['Nf']) == (65, 3, 37)
    for prec in ('f32', 'f64'):
        a, _ = run_case(c, prec)
        b, _ = run_case(c, prec)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_output_holds_exactly_its_rows():
    """the forward writes into a NaN-filled buffer with a margin on either side: every output row is written in full, the
    margins stay NaN; the data rows that the table does not read get a zero gradient"""
    from bayeslim_amd import ops
    c = reference('n33')
    T = lambda a: torch.as_tensor(a, device=DEV).to(torch.complex64)
    X, D, data = T(c['X']), T(c['D']), T(c['data'])
    plan = ops.CouplingPlan(c['table'], c['out_rows'], data.shape[0])
    Nout, Nt, Nf = plan.Nout, c['Nt'], c['Nf']
    buf = torch.empty((Nout + 2, Nt, Nf), dtype=torch.complex64, device=DEV)
    torch.view_as_real(buf).fill_(float('nan'))
    x0, d0 = X.clone(), data.clone()
    out = ops._coupling_fwd_call(X, D, data, plan, c['add_I'], c['prod'], out=buf[1:-1])
    assert out.data_ptr() == buf[1].data_ptr()
    assert bool(torch.isnan(torch.view_as_real(buf[0])).all()) and bool(torch.isnan(torch.view_as_real(buf[-1])).all())
    assert bool(torch.isfinite(torch.view_as_real(buf[1:-1])).all())
    assert torch.equal(out, ops.coupling_apply(X, D, data, plan, add_I=c['add_I'], prod=c['prod']))
    assert torch.equal(X, x0) and torch.equal(data, d0)
    # two more data rows than the table reads
    wide = torch.cat([data, data[:2]]).requires_grad_(True)
    plan2 = ops.CouplingPlan(c['table'], c['out_rows'], wide.shape[0])
    assert plan2.unread
    W = ops.coupling_apply(X, D, wide, plan2, add_I=c['add_I'], prod=c['prod'])
    assert torch.equal(W, out)
    W.abs().sum().backward()
    assert bool((wide.grad[-2:] == 0).all()) and bool((wide.grad[:-2] != 0).any())


def test_no_grad_saves_nothing_and_module_caches():
    import copy
    import pickle
    m, vd, data, kw = golden_setup('both_I_sgl_pt', dtype=torch.float32)
    vd.data = vd.data.detach().to(torch.complex64)
    with torch.no_grad():
        v0 = m(vd)
    assert v0.data.grad_fn is None and not v0.data.requires_grad
    v1 = m(vd)
    assert v1 is v0 and m._vd is v0 and v1.data.requires_grad          # the cached output object, new data
    p0 = m.params.detach().clone()
    v1.data.abs().sum().backward()
    assert torch.equal(m.params.detach(), p0) and m.params.grad.shape == m.params.shape
    assert float(m.params.grad.abs().max()) > 0
    for other in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert torch.equal(other(vd).data, v1.data)
    m.clear_vd_cache()
    assert m._vd is None
    # the keyword decides, self.double only for None
    m.double = True
    assert torch.equal(m(vd).data, v1.data)
    assert not torch.equal(m(vd, double=None).data, v1.data)
    assert torch.equal(m(vd, double=None).data, m(vd, double=True).data)


def test_deepcopy_after_backward():
    """hex-7, 2 times, 3 channels: a deep copy taken after forward and backward holds no cached output and computes the same
    bits; the original's cached output is untouched"""
    import calterm_common as ct
    ct.check_deepcopy_after_backward('VisCoupling', DEV)


def test_chain_in_logprob_and_identity_coupling():
    """Sequential(RedVisModel -> VisCoupling -> JonesModel) in optim.LogProb on hex-7: closure() gives a finite loss and finite,
    non-zero gradients of all three parameter tensors; with X = 0 and add_I the coupling stage returns its input bit for bit"""
    import redcal_common as rc
    from bayeslim_amd import calibration as cal, dataset, optim, utils
    g = rc.golden()
    rng = np.random.default_rng(12)
    ants = [int(a) for a in g['ants']]
    antpos = utils.AntposDict(ants, g['antvecs'])
    bls = [tuple(int(x) for x in b) for b in g['bls']]
    red, Nred = g['red'], int(g['Nred'])
    Nbl, Nant, Nt, Nf = len(bls), len(ants), 3, 5
    cx = lambda *s: torch.as_tensor(rng.normal(size=s) + 1j * rng.normal(size=s))
    times, freqs = torch.as_tensor(g['times']), torch.as_tensor(g['freqs'])

    def vdata(d):
        vd = dataset.VisData()
        vd.setup_meta(None, antpos)
        vd.setup_data(bls, times, freqs, pol='ee', data=d.to(DEV))
        return vd

    data = cx(1, 1, Nbl, Nt, Nf)
    rv = cal.RedVisModel(torch.view_as_real(cx(1, 1, Nred, Nt, Nf)).clone().to(DEV), {bl: int(r) for bl, r in zip(bls, red)},
                         R=cal.VisModelResponse(param_type='com', device=DEV))
    cp = cal.VisCoupling(torch.view_as_real(0.05 * cx(1, 1, Nant, Nant, 1, Nf)).clone().to(DEV), freqs.to(DEV), antpos, bls,
                         R=cal.VisModelResponse(param_type='com', device=DEV))
    cp.setup_coupling(min_dly=2.0)
    jm = cal.JonesModel(torch.view_as_real(torch.exp(0.05 * cx(1, 1, Nant, Nt, Nf))).clone().to(DEV), ants,
                        R=cal.JonesResponse(param_type='com', device=DEV))
    model = utils.Sequential(dict(redvis=rv, coupling=cp, cal=jm))
    prob = optim.LogProb(model, dataset.Dataset([vdata(data)]), start_inp=[vdata(torch.zeros_like(data))], device=DEV)
    loss = prob.closure()
    assert np.isfinite(float(loss)) and float(loss) > 0
    for mod in (rv, cp, jm):
        assert mod.params.grad is not None and bool(torch.isfinite(mod.params.grad).all())
        assert float(mod.params.grad.abs().max()) > 0
    with torch.no_grad():
        cp.params.zero_()
        vin = vdata(data)
        for dt in (torch.complex128, torch.complex64):
            vin.data = vin.data.to(dt)
            cp.clear_vd_cache()
            assert torch.equal(cp(vin, add_I=True).data, vin.data)


def test_left_product_without_a_workspace():
    """prod 'left' at N = 2, Nt = Nf = 1 needs no workspace in either direction: the kernels get the null pointer and zero
    bytes.  W = (I + X) V and both gradients against torch in complex128: sums of two products of numbers of order one, so
    64 roundings of 2^-53 on a magnitude below 16 bound every element."""
    from bayeslim_amd import ops
    from bayeslim_amd._lib import lib
    for stage in (0, 1):
        assert lib.rime_coupling_workspace(ops.RIME_F64, 2, 1, 1, 1, 1, ops.COUPLING_PROD['left'], stage) == 0
    rng = np.random.default_rng(7)
    cx = lambda *s: torch.as_tensor(rng.uniform(-1, 1, size=s) + 1j * rng.uniform(-1, 1, size=s))
    X, d, w = cx(2, 2, 1, 1), cx(3, 1, 1), cx(4, 1, 1)
    table, out_rows = [[0, 1], [1 | ops.COUPLING_CONJ, 2]], [0, 1, 2, 3]

    def ref(X, d):
        V = torch.stack([torch.stack([d[0], d[1]]), torch.stack([d[1].conj(), d[2]])])          # (2, 2, 1, 1)
        E = torch.eye(2, dtype=X.dtype)[:, :, None, None] + X
        return torch.einsum('abtf,bctf->actf', E, V).reshape(4, 1, 1)

    Xr, dr = X.clone().requires_grad_(True), d.clone().requires_grad_(True)
    out_r = ref(Xr, dr)
    gXr, gdr = torch.autograd.grad((out_r * w.conj()).real.sum(), [Xr, dr])
    Xg, dg = X.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
    out = ops.coupling_apply(Xg, None, dg, table, out_rows, prod='left')
    gX, gd = torch.autograd.grad((out * w.to(DEV).conj()).real.sum(), [Xg, dg])
    tol = 64 * 2.0 ** -53 * 16
    for a, b in ((out, out_r), (gX, gXr), (gd, gdr)):
        assert a.shape == b.shape and a.dtype == torch.complex128 and float((a.detach().cpu() - b.detach()).abs().max()) <= tol
