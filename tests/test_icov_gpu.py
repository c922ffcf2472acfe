"""
The fused axis-covariance kernel (csrc/icov.hip) on the GPU against the float64 oracle of icov_common.py: the raw (O, n, I)
problem in both precisions over every planner branch, ops.chisq_axis and its gradients for every cov_axis, and the public
path optim.forward_chisq / LogProb.forward_like with targets that carry an axis covariance.  Bounds: icov_common.bound.
"""
import numpy as np
import pytest
import torch

import icov_common as ic

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.complex64, torch.complex128]
DT_IDS = ['c64', 'c128']


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from bayeslim_amd import ops
    return ops


def run_raw(ops, O, n, I, dtype, want=(True, True, True)):
    """(y, q, total) of the kernel on the raw problem, all three outputs of one launch (None where not wanted)"""
    P = ic.raw_problem(O, n, I, dtype)
    p, d, w = P['pred'].to(DEV), P['data'].to(DEV), P['W'].to(DEV).reshape(O * I, n, n).contiguous()
    rdt = torch.float32 if dtype == torch.complex64 else torch.float64
    y = torch.full((O, n, I), float('nan'), dtype=dtype, device=DEV) if want[0] else None
    q = torch.full((O, I), float('nan'), dtype=rdt, device=DEV) if want[1] else None
    out = torch.full((), float('nan'), dtype=rdt, device=DEV) if want[2] else None
    ops._icov_fwd_call(p, d, w, O, n, I, y, q, out)
    torch.cuda.synchronize()
    return y, q, out


def check_raw(ops, O, n, I, dtype):
    P = ic.raw_problem(O, n, I, dtype)
    y, q, out = run_raw(ops, O, n, I, dtype)
    ey = (y.cpu().to(torch.complex128) - P['y']).abs()
    eq = (q.cpu().double() - P['q']).abs()
    et = abs(float(out.cpu().double()) - float(P['q'].sum()))
    by, bq, bt = ic.bound(n, dtype, P['Srow']), ic.bound(n, dtype, P['S']), float(ic.bound(n, dtype, P['S'].sum()))
    print('O=%d n=%d I=%d %s: y %.3g of bound, q %.3g, total %.3g' % (O, n, I, dtype, float((ey / by).max()),
                                                                     float((eq / bq).max()), et / bt))
    assert bool((ey <= by).all()) and bool((eq <= bq).all()) and et <= bt
    # determinism: a second launch returns the same bits; outputs that are not wanted change nothing in the others
    y2, q2, out2 = run_raw(ops, O, n, I, dtype)
    assert torch.equal(y, y2) and torch.equal(q, q2) and torch.equal(out, out2)
    _, _, out3 = run_raw(ops, O, n, I, dtype, want=(False, False, True))
    _, q3, _ = run_raw(ops, O, n, I, dtype, want=(False, True, False))
    assert torch.equal(out, out3) and torch.equal(q, q3)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('shape', ic.RAW_SHAPES, ids=lambda s: 'O%d-n%d-I%d' % s)
def test_raw_problem_against_float64(ops, shape, dtype):
    check_raw(ops, *shape, dtype)


@pytest.mark.parametrize('shape', ic.RAW_SHAPES_C64, ids=lambda s: 'O%d-n%d-I%d' % s)
def test_raw_problem_complex64_only(ops, shape):
    """(1, 257, 9): a ragged second tile at the longest rows (icov_common: the pruning rule of the raw shapes)"""
    assert ops.icov_plan(torch.complex64, *shape)['tile'] == 8
    check_raw(ops, *shape, torch.complex64)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_few_large_batches_split_their_rows(ops, dtype):
    O, n, I = ic.SPLIT_SHAPE
    plan = ops.icov_plan(dtype, O, n, I)
    assert plan['splits'] > 1 and plan['grid'] == O * I * plan['splits']
    check_raw(ops, O, n, I, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_more_tiles_than_the_capped_grid(ops, dtype):
    O, n, I = ic.CAPPED_SHAPE
    plan = ops.icov_plan(dtype, O, n, I)
    assert plan['grid'] == 4096 < O * -(-I // plan['tile']) * plan['splits']
    check_raw(ops, O, n, I, dtype)


def _oracle_autograd(case, pred, data, icov, cot=None):
    """float64 autograd of the oracle: gradient of sum(q) or of sum(cot q) w.r.t. pred"""
    p = pred.to(torch.complex128).clone().requires_grad_(True)
    q = ic.oracle_einsum(case, p - data.to(torch.complex128), icov)
    (q.sum() if cot is None else (q * cot).sum()).backward()
    return q.detach(), p.grad


def _bound_terms(case, pred, data, icov):
    """S per batch (output shape) and sum_c |W_ac| |r_c| per data element, float64"""
    mode, cov_axis = ic.CASES[case][:2]
    r = (pred.to(torch.complex128) - data.to(torch.complex128)).abs().to(torch.complex128)
    Wa = icov.to(torch.complex128).abs().to(torch.complex128)
    S = torch.einsum(ic.CASES[case][5], r, Wa, r).real
    eq = ic.CASES[case][5]
    lhs, out = eq.split('->')
    _, w_idx, r_idx = lhs.split(',')
    row_idx = lhs.split(',')[0]                                    # the conjugated operand's indices: the data's own
    Srow = torch.einsum('%s,%s->%s' % (w_idx, r_idx, row_idx), Wa, r).real
    return S, Srow


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('case', range(len(ic.CASES)), ids=ic.CASE_IDS)
def test_chisq_axis_values_and_gradients(ops, case, dtype):
    mode, cov_axis, shape, icov_shape, out_shape, _ = ic.CASES[case]
    pred, data, icov = ic.public_problem(case, dtype)
    n = icov_shape[-1]
    S, Srow = _bound_terms(case, pred, data, icov)
    rdt = torch.float32 if dtype == torch.complex64 else torch.float64
    p = pred.to(DEV).requires_grad_(True)
    d, w = data.to(DEV), icov.to(DEV)
    # summed
    tot = ops.chisq_axis(p, d, w, cov_axis, mode=mode)
    assert tot.shape == () and tot.dtype == rdt and tot.requires_grad
    q64, g64 = _oracle_autograd(case, pred, data, icov)
    assert abs(float(tot.detach()) - float(q64.sum())) <= float(ic.bound(n, dtype, S.sum()))
    g, = torch.autograd.grad(tot, p)
    assert g.shape == shape and g.dtype == dtype
    assert bool(((g.cpu().to(torch.complex128) - g64).abs() <= 2 * ic.bound(n, dtype, Srow)).all())
    # per batch, with a random cotangent
    per = ops.chisq_axis(p, d, w, cov_axis, mode=mode, sum_chisq=False)
    assert per.shape == out_shape and per.dtype == rdt
    assert bool(((per.detach().cpu().double() - q64).abs() <= ic.bound(n, dtype, S)).all())
    cot = torch.as_tensor(np.random.default_rng(5).normal(size=out_shape)).to(rdt)
    _, gc64 = _oracle_autograd(case, pred, data, icov, cot.double())
    gc, = torch.autograd.grad(per, p, cot.to(DEV))
    cot_el = cot.double().abs().unsqueeze(ic.AXIS[(mode, cov_axis)]).expand(shape)
    assert bool(((gc.cpu().to(torch.complex128) - gc64).abs() <= 2 * cot_el * ic.bound(n, dtype, Srow)).all())
    # determinism, and no_grad (which keeps no product) returns the same bits
    assert torch.equal(tot.detach(), ops.chisq_axis(p, d, w, cov_axis, mode=mode).detach())
    with torch.no_grad():
        t0 = ops.chisq_axis(p, d, w, cov_axis, mode=mode)
        per0 = ops.chisq_axis(p, d, w, cov_axis, mode=mode, sum_chisq=False)
    assert not t0.requires_grad and torch.equal(t0, tot.detach()) and torch.equal(per0, per.detach())
    assert torch.equal(ops.chisq_axis(p.detach(), d, w, cov_axis, mode=mode), tot.detach())
    # broadcastable data, and none
    d1 = d[:1]
    ref = ic.oracle_einsum(case, pred - data[:1], icov)
    S1, _ = _bound_terms(case, pred, data[:1].expand(shape), icov)
    assert abs(float(ops.chisq_axis(p, d1, w, cov_axis, mode=mode).detach()) - float(ref.sum())) <= float(ic.bound(n, dtype, S1.sum()))
    S0, _ = _bound_terms(case, pred, torch.zeros_like(pred), icov)
    ref0 = ic.oracle_einsum(case, pred, icov)
    assert abs(float(ops.chisq_axis(p, None, w, cov_axis, mode=mode).detach()) - float(ref0.sum())) <= float(ic.bound(n, dtype, S0.sum()))
    with pytest.raises(ValueError):
        ops.chisq_axis(p, d, w[..., :-1, :], cov_axis, mode=mode)
    with pytest.raises(ValueError):
        ops.chisq_axis(p, d, w.clone().requires_grad_(True), cov_axis, mode=mode)


def test_icov_of_another_dtype_is_converted_with_one_warning(ops):
    case = ic.CASE_IDS.index('vis-freq')
    pred, data, icov = ic.public_problem(case, torch.complex64)
    p, d, w = pred.to(DEV), data.to(DEV), icov.to(DEV)
    ops._ChisqAxis._warned = False
    with pytest.warns(UserWarning, match="store it in the prediction's dtype"):
        a = ops.chisq_axis(p, d, w.to(torch.complex128), 'freq')
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        b = ops.chisq_axis(p, d, w.to(torch.complex128), 'freq')       # once only
        c = ops.chisq_axis(p, d, w, 'freq')
    assert torch.equal(a, b) and torch.equal(a, c)


def test_diagonal_path_is_unchanged(ops):
    """cov_axis None through forward_chisq is ops.chisq, bit for bit, as before the axis covariances"""
    from bayeslim_amd import optim
    pred, data, _ = ic.public_problem(2, torch.complex64)
    p, d = pred.to(DEV), data.to(DEV)
    w = torch.rand(p.shape, device=DEV)
    a, res = optim.forward_chisq(p, d, w, None)
    assert res is None and torch.equal(a, ops.chisq(p, d, w)) and torch.equal(a, optim.forward_chisq(p, d, w)[0])
    b, res = optim.forward_chisq(p, d, None, None, sum_chisq=False)
    assert torch.equal(b, ((p - d).conj() * (p - d)).real) and res is not None


# ---- public path: targets with an axis covariance under optim.forward_chisq and LogProb -----------------------------------
def _c1_model():
    """the 7-antenna point-source RIME of test_rime_gpu.test_rime_c1_point_sources: vis (1, 1, 21, 2, 8)"""
    import test_rime_gpu as trg
    import bayeslim_amd
    from bayeslim_amd import sky_model, beam_model, rime_model
    from conftest import load_golden
    g = load_golden('rime_c1')
    freqs = trg.T(g['freqs'])
    arr, tel = trg.make_array(bayeslim_amd, g, freqs)
    R = sky_model.PointSkyResponse(freqs, freq_mode='powerlaw', f0=freqs[0], device=DEV)
    sky = sky_model.PointSky(trg.T(g['sky_params']), trg.T(np.stack([g['ra'], g['dec']]), torch.float64), R=R, parameter=True,
                             name='ptsky')
    beam = beam_model.PixelBeam(torch.ones(1, 1, 1, 1, 1, device=DEV) * float(g['airy_D']), freqs,
                                R=beam_model.AiryResponse(powerbeam=True), pol='e', powerbeam=True, fov=180, parameter=False)
    sim_bls = [tuple(b) for b in g['sim_bls']]
    rime = rime_model.RIME(sky, tel, beam, arr, sim_bls, g['times'], freqs)
    trg.fill_cache(tel, 'ptsky', g)
    return rime, sim_bls, g, freqs


def _check_like(prob, target, pred, data, case_einsum, n, dtype):
    """forward_chisq returns (chisq, None); forward_like agrees with chisq + cov_ndim log(pi) + logdet in float64"""
    from bayeslim_amd import optim
    chisq, res = prob.forward_chisq()
    assert res is None and not chisq.is_complex() and chisq.shape == ()
    r = (pred.detach().cpu().to(torch.complex128) - data.cpu().to(torch.complex128))
    W = target.icov.cpu().to(torch.complex128)
    ref = float(torch.einsum(case_einsum, r.conj(), W, r).real.sum())
    S = float(torch.einsum(case_einsum, r.abs().to(W.dtype), W.abs().to(W.dtype), r.abs().to(W.dtype)).real.sum())
    bnd = float(ic.bound(n, dtype, torch.tensor(S)))
    assert abs(float(chisq) - ref) <= bnd
    c2, res2 = optim.forward_chisq(pred.detach(), data, target.icov, target.cov_axis,
                                   mode='map' if case_einsum.startswith('ijkl,') else 'vis')
    assert res2 is None and torch.equal(c2, chisq.detach())
    like = prob.forward_like()
    logpi, logdet = target.cov_ndim * np.log(np.pi), float(target.cov_logdet.double())
    want = ref + logpi + logdet
    # the normalisation is added to the chi-square in the working precision: a rounding of each term and of each sum
    assert abs(float(like) - want) <= bnd + 4 * ic.UNIT[dtype] * (abs(ref) + abs(logpi) + abs(logdet))
    return like


@pytest.mark.parametrize('cov_axis', ['freq', 'time', 'bl'])
def test_logprob_with_an_axis_covariance_on_a_visdata_target(ops, cov_axis):
    from bayeslim_amd import optim, dataset, utils
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    try:
        rime, sim_bls, g, freqs = _c1_model()
        dtype = torch.complex64
        vis = torch.as_tensor(g['vis']).to(dtype)
        Nbl, Nt, Nf = vis.shape[2:]
        case = ic.CASE_IDS.index('vis-' + cov_axis)
        _, O, n, I, cov_shape, _ = ops.cov_axis_layout(vis.shape, cov_axis, 'vis')
        rng = np.random.default_rng(11)
        scale = float(vis.abs().mean()) ** 2
        cov = torch.as_tensor(ic.hermitian_pd(rng, cov_shape[:-2], n) * (scale / n)).to(dtype).to(DEV)
        data = (vis + 0.1 * float(vis.abs().mean()) * torch.as_tensor(ic.cnormal(rng, vis.shape)).to(dtype)).to(DEV)
        target = dataset.VisData()
        target.setup_data(sim_bls, torch.as_tensor(g['times']), freqs, pol='ee', data=data)
        target.set_cov(cov, cov_axis)
        target.compute_icov()
        assert target.icov.shape == cov_shape and target.cov_ndim == vis.numel()
        prob = optim.LogProb(utils.Sequential(dict(rime=rime)), dataset.Dataset([target]), device=DEV)
        pred = rime().data
        like = _check_like(prob, target, pred, data, ic.CASES[case][5], n, dtype)
        assert like.requires_grad
        loss = prob.closure()                                           # the gradient reaches the sky through the saved product
        assert torch.isfinite(loss).all() and float(rime.sky.params.grad.abs().max()) > 0
    finally:
        torch.set_default_dtype(old)


def test_logprob_with_a_pixel_covariance_on_a_mapdata_target(ops):
    from bayeslim_amd import optim, dataset, utils
    case = ic.CASE_IDS.index('map-pix')
    dtype = torch.complex64
    pred0, data, cov = ic.public_problem(case, dtype)

    class Map(utils.Module):
        def __init__(self):
            super().__init__(name='map')
            self.params = torch.nn.Parameter(pred0.to(DEV))

        def forward(self, inp=None, prior_cache=None, **kw):
            md = dataset.MapData()
            md.data = self.params * 1.0
            return md

    target = dataset.MapData()
    target.setup_data(torch.linspace(1e8, 2e8, 6), data=data.to(DEV))
    target.set_cov(cov.to(DEV), 'pix')
    target.compute_icov()
    model = Map()
    prob = optim.LogProb(model, dataset.Dataset([target]), device=DEV)
    _check_like(prob, target, model.params, data.to(DEV), ic.CASES[case][5], 7, dtype)
    prob.closure()
    _, g64 = _oracle_autograd(case, pred0, data, target.icov.cpu())
    _, Srow = _bound_terms(case, pred0, data, target.icov.cpu())
    assert bool(((model.params.grad.cpu().to(torch.complex128) - g64).abs() <= 2 * ic.bound(7, dtype, Srow)).all())
