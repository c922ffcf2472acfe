"""
The fused log-prior kernel (csrc/prior.hip) on the GPU against the float64 oracle of prior_common.py, within
prior_common.bound: every kind in both precisions over the sizes at which the lane layout changes (a ragged last group, a
second chunk, a second trip of the grid-stride loop), every operand mode, side, choice of bounds and alpha, misaligned
tensors bit for bit, and the public path through optim.LogProb.
"""
import numpy as np
import pytest
import torch

import prior_common as pc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.float32, torch.float64]
DT_IDS = ['f32', 'f64']


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from bayeslim_amd import ops
    return ops


def dev(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(dtype).to(DEV)


def case(kind, N, i=0, shape=None, mode='scalar', side=None, bounds=None, alpha=None):
    """(x, operand keywords, side) of the i-th variant of a kind: side, bounds and alpha cycle with i unless given"""
    if kind == 'laplace':
        x, m, s = pc.laplace_case(N, seed=i, shape=shape, mode=mode)
        return x, dict(mean=m, scale=s), side or pc.SIDES[i % 3]
    x, lo, hi, c = pc.taper_case(N, kind, bounds or pc.BOUNDS[i % 3], alpha or pc.ALPHAS[i % 2], seed=i, shape=shape, mode=mode)
    return x, dict(lower=lo, upper=hi, coeff=c), 'both'


def evaluate(ops, kind, x, kw, side, dtype, g=1.0):
    p = dev(x, dtype).requires_grad_(True)
    val = ops.prior_eval(kind, p, side=side, **{k: dev(v, dtype) for k, v in kw.items()})
    assert val.shape == () and val.dtype == dtype and val.requires_grad
    (g * val).backward()
    return val.detach(), p.grad


def check(ops, kind, x, kw, side, dtype, g=1.0, what=''):
    o = pc.oracle(kind, x, side=side, **kw)
    val, grad = evaluate(ops, kind, x, kw, side, dtype, g)
    bv, bg = pc.bound(kind, dtype, o, g)
    ev = abs(float(val.double()) - o['value'])
    eg = np.abs(grad.cpu().double().numpy() - g * o['grad'])
    ok = bg > 0
    print('%s %s %s N=%d %s: value %.3g of bound, gradient %.3g' % (kind, dtype, side, x.size, what, ev / bv,
                                                                   float((eg[ok] / bg[ok]).max()) if ok.any() else 0.0))
    assert np.isfinite(o['value']) and ev <= bv
    assert bool(np.all(eg <= bg))
    return val, grad


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('N', pc.SIZES)
@pytest.mark.parametrize('kind', pc.KINDS)
def test_sizes_against_float64(ops, kind, N, dtype):
    i = pc.SIZES.index(N)
    for mode in ('scalar', 'full'):
        x, kw, side = case(kind, N, i, mode=mode)
        val, grad = check(ops, kind, x, kw, side, dtype, what=mode)
        val2, grad2 = evaluate(ops, kind, x, kw, side, dtype)                  # two launches: the same bits
        assert torch.equal(val, val2) and torch.equal(grad, grad2)
        if kind == 'laplace':                                                  # residuals that are exactly 0: gradient 0
            assert bool((grad[::8] == 0).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_every_side_bounds_and_alpha_with_an_upstream_gradient(ops, dtype):
    for side in pc.SIDES:
        x, kw, _ = case('laplace', 257, 1, mode='full', side=side)
        check(ops, 'laplace', x, kw, side, dtype, g=2.5)
    for kind in ('taper_sigmoid', 'taper_tanh'):
        for bounds in pc.BOUNDS:
            for alpha in pc.ALPHAS:
                x, kw, _ = case(kind, 257, 2, mode='scalar', bounds=bounds, alpha=alpha)
                check(ops, kind, x, kw, 'both', dtype, g=2.5, what='%s alpha %g' % (bounds, alpha))


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('kind', pc.KINDS)
def test_second_trip_of_the_grid_stride_loop(ops, kind, dtype):
    N = ops.prior_grid_span(dtype) + 65                      # one full grid of chunks and a ragged chunk for block 0
    assert 10 ** 6 < N < 10 ** 7
    x, kw, side = case(kind, N, 3, mode='scalar')
    check(ops, kind, x, kw, side, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('kind', pc.KINDS)
def test_trailing_periods(ops, kind, dtype):
    for shape, mode in (((7, 3), 3), ((4, 2, 5), 5), ((4, 2, 5), 10)):
        x, kw, side = case(kind, None, 4, shape=shape, mode=mode)
        assert all(v is None or v.size == mode for v in kw.values())
        check(ops, kind, x, kw, side, dtype, what='period %d of %s' % (mode, shape))


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('kind', pc.KINDS)
def test_one_element_off_a_16_byte_boundary_gives_the_same_bits(ops, kind, dtype):
    for N in (65, 4097):
        x, kw, side = case(kind, N, 5, mode='full')
        val, grad = evaluate(ops, kind, x, kw, side, dtype)

        def off(a):
            if a is None:
                return None
            buf = torch.empty(N + 1, dtype=dtype, device=DEV)
            assert buf.data_ptr() % 16 == 0
            buf[1:] = dev(a, dtype)
            return buf[1:]
        p = off(x).requires_grad_(True)
        assert p.data_ptr() % 16 != 0 and p.is_contiguous()
        v2 = ops.prior_eval(kind, p, side=side, **{k: off(v) for k, v in kw.items()})
        v2.backward()
        assert torch.equal(val, v2.detach()) and torch.equal(grad, p.grad)
        # ... and the derivative stored off the boundary (the private call: autograd's buffer is always aligned)
        dbuf = torch.full((N + 2,), float('nan'), dtype=dtype, device=DEV)
        operands = [None if kw.get(k) is None else off(kw[k]) for k in ('mean', 'scale', 'lower', 'upper', 'coeff')]
        out = torch.empty((), dtype=dtype, device=DEV)
        ops._prior_fwd_call(kind, side, p.detach(), operands, out, dbuf[1:N + 1])
        assert torch.equal(out, val) and torch.equal(dbuf[1:N + 1], grad) and bool(torch.isnan(dbuf[[0, N + 1]]).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_no_grad_call_stores_no_derivative(ops, dtype):
    N = 257
    x, kw, side = case('taper_sigmoid', N, 0, mode='scalar')
    xs = dev(x, dtype)
    operands = [None, None] + [dev(kw[k], dtype) for k in ('lower', 'upper', 'coeff')]
    buf = torch.full((2 * N,), float('nan'), dtype=dtype, device=DEV)
    out0 = torch.empty((), dtype=dtype, device=DEV)
    ops._prior_fwd_call('taper_sigmoid', side, xs, operands, out0, None)       # the null derivative pointer
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    out1 = torch.empty((), dtype=dtype, device=DEV)
    ops._prior_fwd_call('taper_sigmoid', side, xs, operands, out1, buf[:N])
    torch.cuda.synchronize()
    assert torch.equal(out0, out1) and bool(torch.isfinite(buf[:N]).all()) and bool(torch.isnan(buf[N:]).all())
    with torch.no_grad():
        v = ops.prior_eval('taper_sigmoid', xs.clone().requires_grad_(True), side=side, lower=operands[2], upper=operands[3],
                           coeff=operands[4])
    assert not v.requires_grad and torch.equal(v, out0)
    assert torch.equal(ops.prior_eval('taper_sigmoid', xs, lower=operands[2], upper=operands[3], coeff=operands[4]), out0)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_tanh_taper_outside_its_bounds_is_nan(ops, dtype):
    x, kw, _ = case('taper_tanh', 257, 0, mode='scalar', bounds='both', alpha=1.0)
    inside = pc.oracle('taper_tanh', x, **kw)
    x = x.copy()
    x[100] = pc.HI + 1.0
    x[200] = pc.LO - 0.5
    assert np.isnan(pc.oracle('taper_tanh', x, **kw)['value'])
    val, grad = evaluate(ops, 'taper_tanh', x, kw, 'both', dtype)
    torch.cuda.synchronize()
    assert bool(torch.isnan(val))
    keep = np.ones(257, dtype=bool)
    keep[[100, 200]] = False
    _, bg = pc.bound('taper_tanh', dtype, inside)
    assert bool(np.all(np.abs(grad.cpu().double().numpy() - inside['grad'])[keep] <= bg[keep]))


# ---- public path ----------------------------------------------------------------------------------------------------------
def _logprob(device, dtype, x0, priors):
    from bayeslim_amd import optim, dataset, utils

    class Par(utils.Module):
        def __init__(self):
            super().__init__(name='par')
            self.params = torch.nn.Parameter(torch.as_tensor(x0).to(dtype).to(device))

        def forward(self, inp=None, prior_cache=None, **kw):
            self.eval_prior(prior_cache)
            return self.params

    model = Par()
    model.set_priors(priors_inp_params=priors)
    for p in priors:
        p.push(device)
        p.push(torch.float32 if dtype in (torch.float32, torch.complex64) else torch.float64)
    target = dataset.MapData()
    target.setup_data(torch.linspace(1e8, 2e8, 2), data=torch.zeros(1, 1, 2, 3, device=device))
    prob = optim.LogProb(model, dataset.Dataset([target]), device=device, compute='prior')
    prob.set_main_params(['params'])
    return prob


def _evaluate_logprob(prob, default_dtype):
    """(forward_prior, closure loss) with the default dtype LogProb creates its accumulators in"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(default_dtype)
    try:
        return prob.forward_prior().detach(), prob.closure()
    finally:
        torch.set_default_dtype(old)


def test_logprob_with_the_new_priors_against_float64_on_the_cpu(ops):
    from bayeslim_amd import optim
    x, m, s = pc.laplace_case(None, seed=7, shape=(6, 5), mode=5)
    xt, lo, hi, c = pc.taper_case(None, 'taper_sigmoid', 'both', 8.0, seed=7, shape=(2, 5), mode='scalar')
    x[2:4] = xt                                                                # the indexed slice sits in the taper's range
    idx = (slice(2, 4),)

    def priors():
        return [optim.LogLaplacePrior(torch.as_tensor(m), torch.as_tensor(s), side='upper'),
                optim.LogTaperedUniformPrior(torch.as_tensor(lo), torch.as_tensor(hi), alpha=8.0, index=idx)]

    gpu = _logprob(DEV, torch.float32, x, priors())
    cpu = _logprob('cpu', torch.float64, x, priors())
    pr = gpu.model.priors_inp_params
    assert ops.prior_fits(gpu.model.params, (pr[0].mean, pr[0].scale))
    assert ops.prior_fits(gpu.model.params[idx], (pr[1].lower_bound, pr[1].upper_bound, pr[1].coeff))
    assert float(pr[1].coeff) == 2.0
    (vg, lg), (vc, lc) = _evaluate_logprob(gpu, torch.float32), _evaluate_logprob(cpu, torch.float64)
    o1 = pc.oracle('laplace', x, m, s, side='upper')
    o2 = pc.oracle('taper_sigmoid', x[2:4], lower=lo, upper=hi, coeff=c)
    b1, g1 = pc.bound('laplace', torch.float32, o1)
    b2, g2 = pc.bound('taper_sigmoid', torch.float32, o2)
    norm = float(np.sum(np.log(2 * s)))
    # each prior within its bound, then the norm and the additions of the cache in float32: a rounding each
    mag = abs(o1['value']) + norm + abs(o2['value'])
    tol = b1 + b2 + 4 * pc.EPS[torch.float32] * mag
    assert abs(float(vc) - -(o1['value'] - norm + o2['value'])) <= 1e-12 * mag
    assert vg.dtype == torch.float32 and abs(float(vg) - float(vc)) <= tol and abs(float(lg) - float(lc)) <= tol
    bg = g1.copy()
    bg[2:4] += g2 + 0.5 * pc.EPS[torch.float32] * (o1['abs_d'][2:4] + o2['abs_d'])       # the two gradients are added
    err = np.abs(gpu.main_params.grad.cpu().double().numpy() - cpu.main_params.grad.numpy())
    assert err.shape == (30,) and bool(np.all(err <= bg.ravel()))
    assert float(cpu.main_params.grad.abs().max()) > 0


def test_complex_parameter_with_a_laplace_prior_takes_the_torch_path(ops):
    from bayeslim_amd import optim
    rng = np.random.default_rng(3)
    z = rng.normal(size=(4, 3)) + 1j * rng.normal(size=(4, 3))

    def priors():
        return [optim.LogLaplacePrior(torch.tensor(0.25 + 0.5j, dtype=torch.complex128), torch.tensor(2.0, dtype=torch.float64))]

    gpu = _logprob(DEV, torch.complex128, z, priors())
    cpu = _logprob('cpu', torch.complex128, z, priors())
    pr = gpu.model.priors_inp_params[0]
    assert gpu.model.params.is_cuda and not ops.prior_fits(gpu.model.params, (pr.mean, pr.scale))
    (vg, _), (vc, _) = _evaluate_logprob(gpu, torch.float64), _evaluate_logprob(cpu, torch.float64)
    want = np.sum(np.abs(z - (0.25 + 0.5j))) / 2 + np.log(4.0)
    assert abs(float(vc) - want) <= 1e-12 * want and abs(float(vg) - want) <= 1e-12 * want
    assert torch.allclose(gpu.main_params.grad.cpu(), cpu.main_params.grad, rtol=1e-12, atol=1e-14)
