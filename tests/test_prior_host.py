"""
LogLaplacePrior and LogTaperedUniformPrior without a GPU: the torch compositions against the recorded reference
(tests/golden/prior.npz) and the float64 oracle of prior_common.py, their gradients, the BaseLogPrior plumbing, and the
argument checks of rime_prior_fwd / rime_prior_bwd, which come before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_asm
import prior_common as pc
from conftest import load_golden


def T(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)


def build(cls, kw, dtype=torch.float64):
    from bayeslim_amd import optim
    if cls == 'laplace':
        return optim.LogLaplacePrior(T(kw['mean'], dtype), T(kw['scale'], dtype), side=kw['side'], density=kw['density'])
    return optim.LogTaperedUniformPrior(T(kw['lower_bound'], dtype), T(kw['upper_bound'], dtype), kind=kw['kind'],
                                        alpha=torch.as_tensor(kw['alpha'], dtype=dtype))


def close(a, b, rtol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1e-300)))


GOLDEN_CASES = pc.golden_cases()


@pytest.mark.parametrize('case', GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_cpu_values_and_gradients_against_the_reference_and_the_oracle(case):
    name, cls, kw, x = case
    g = load_golden('prior')
    assert np.array_equal(g[name + '_x'], x)
    prior = build(cls, kw)
    p = T(x).clone().requires_grad_(True)
    before = p.detach().clone()
    val = prior(p)
    val.backward()
    assert torch.equal(p.detach(), before)                           # params is not modified
    assert val.dtype == torch.float64 and val.shape == ()
    # the value to 1e-12 of the sum of the terms' magnitudes (alpha = 1e4 sums to nearly nothing), the gradient per element
    if cls == 'laplace':
        o = pc.oracle('laplace', x, kw['mean'], kw['scale'], side=kw['side'])
        norm = float(np.sum(np.log(2 * np.atleast_1d(kw['scale'])))) if kw['density'] else 0.0
        want = o['value'] - norm
    else:
        c = kw['alpha'] / (pc.HI - pc.LO) if kw['lower_bound'] is not None and kw['upper_bound'] is not None else kw['alpha']
        o = pc.oracle('taper_' + kw['kind'], x, lower=kw['lower_bound'], upper=kw['upper_bound'], coeff=c)
        want = o['value']
    scale = max(float(o['abs_t'].sum()), abs(want))
    assert abs(float(val.detach()) - want) <= 1e-12 * scale
    assert abs(float(val.detach()) - float(g[name + '_value'])) <= 1e-12 * scale
    # the oracle element by element; the reference relative to the largest element: its own gradient of log(sigmoid) and
    # log(tanh) loses the small elements to the cancellation in 1 - sigmoid(z) and 1 - tanh(z)^2
    # (so does the torch composition of log(tanh), which is the literal one: there the oracle is met the same way)
    per_element = np.abs(o['grad']).max() if kw.get('kind') == 'tanh' else np.maximum(o['abs_d'], 1e-300)
    assert bool(np.all(np.abs(p.grad.numpy() - o['grad']) <= 1e-12 * per_element))
    assert bool(np.all(np.abs(p.grad.numpy() - g[name + '_grad']) <= 1e-12 * np.abs(o['grad']).max()))


def test_index_func_and_fkwargs():
    from bayeslim_amd import optim
    x, m, s = pc.laplace_case(12, shape=(4, 3), mode=3)
    p = T(x).requires_grad_(True)
    idx = (slice(1, 3),)
    pr = optim.LogLaplacePrior(T(m), T(s), density=False, index=idx, func=lambda a, k=1.0: a * k, fkwargs=dict(k=2.0))
    o = pc.oracle('laplace', 2 * x[1:3], m, s)
    val = pr(p)
    assert close(val.detach(), o['value'])
    val.backward()
    want = np.zeros_like(x)
    want[1:3] = 2 * o['grad']
    assert close(p.grad, want)
    tp = optim.LogTaperedUniformPrior(-8.0, 8.0, alpha=4.0, index=(slice(None), 0))
    assert tp.attrs == ['coeff', 'lower_bound', 'upper_bound'] and pr.attrs == ['mean', 'scale']
    o = pc.oracle('taper_sigmoid', x[:, 0], lower=-8.0, upper=8.0, coeff=0.25)
    assert close(tp(T(x)), o['value'])
    one = optim.LogTaperedUniformPrior(lower_bound=0.5, kind='tanh', alpha=3.0)
    assert one.dbound == 1.0 and float(one.coeff) == 3.0 and one.upper_bound is None
    with pytest.raises(AssertionError):
        optim.LogTaperedUniformPrior()


def test_push_to_a_dtype_and_names():
    from bayeslim_amd import optim
    pr = optim.LogLaplacePrior(torch.zeros(3), torch.ones(3), side='lower')
    assert (pr.side, pr.density) == ('lower', True) and float(pr.norm) == pytest.approx(3 * np.log(2.0))
    pr.push(torch.float64)
    assert pr.mean.dtype == torch.float64 and pr.scale.dtype == torch.float64
    tp = optim.LogTaperedUniformPrior(torch.zeros(3), torch.ones(3), alpha=10.0)
    tp.push(torch.float64)
    assert tp.coeff.dtype == tp.lower_bound.dtype == tp.upper_bound.dtype == torch.float64
    assert (tp.kind, float(tp.alpha)) == ('sigmoid', 10.0) and torch.equal(tp.dbound, torch.ones(3))
    val = tp(torch.full((2, 3), 0.5, dtype=torch.float64))
    assert val.dtype == torch.float64


def test_complex_laplace_residual_and_float32_density():
    from bayeslim_amd import optim
    z = torch.tensor([1 + 1j, -2j, 0.5], dtype=torch.complex128, requires_grad=True)
    pr = optim.LogLaplacePrior(torch.tensor(0.5 + 0j, dtype=torch.complex128), 2.0, density=False)
    val = pr(z)
    assert not val.is_complex() and close(val.detach(), -np.sum(np.abs(np.array([0.5 + 1j, -0.5 - 2j, 0.0]))) / 2)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)            # explicit: the default dtype is the process's, not this test's
    out = optim.LogLaplacePrior(f32(0.0), f32(1.0))(torch.ones(4, dtype=torch.float32))
    assert out.dtype == torch.float32 and float(out) == pytest.approx(-4 - np.log(2.0), rel=1e-6)


def test_stable_log_sigmoid_is_finite_where_the_literal_form_is_not():
    from bayeslim_amd import optim
    tp = optim.LogTaperedUniformPrior(lower_bound=torch.tensor(0.0, dtype=torch.float32), alpha=torch.tensor(1.0, dtype=torch.float32))
    x = torch.tensor([-200.0], dtype=torch.float32, requires_grad=True)
    val = tp(x)
    assert val.dtype == torch.float32 and float(val.detach()) == -200.0
    assert float(torch.log(torch.sigmoid(x.detach()))) == -np.inf            # the reference's literal form
    val.backward()
    assert float(x.grad) == 1.0
    assert float(pc.oracle('taper_sigmoid', [-200.0], lower=0.0, coeff=1.0)['value']) == -200.0


def test_tanh_taper_is_nan_outside_its_bounds():
    from bayeslim_amd import optim
    tp = optim.LogTaperedUniformPrior(0.0, 1.0, kind='tanh', alpha=2.0)
    assert torch.isfinite(tp(torch.tensor([0.25, 0.5], dtype=torch.float64)))
    assert torch.isnan(tp(torch.tensor([0.25, 1.5], dtype=torch.float64)))
    assert torch.isnan(tp(torch.tensor([-0.5, 0.5], dtype=torch.float64)))
    assert np.isnan(pc.oracle('taper_tanh', [0.25, 1.5], lower=0.0, upper=1.0, coeff=2.0)['value'])


def test_prior_fits_refuses_what_the_kernel_does_not_serve():
    from bayeslim_amd import ops
    x = torch.zeros(4, 2, 5)
    assert not ops.prior_fits(x, (1.0,))                                                   # CPU
    P = ops._prior_period
    assert P(x.shape, None) == 0 and P(x.shape, 2.0) == 1 and P(x.shape, torch.ones(1, 1)) == 1
    assert P(x.shape, torch.ones(4, 2, 5)) == 40 and P(x.shape, torch.ones(5)) == 5 and P(x.shape, torch.ones(1, 2, 5)) == 10
    assert P(x.shape, torch.ones(2, 1)) is None and P(x.shape, torch.ones(4, 1, 1)) is None    # a middle / leading axis
    assert P(x.shape, torch.ones(3, 4, 2, 5)) is None and P(x.shape, torch.ones(5, dtype=torch.complex64)) is None
    assert P(x.shape, torch.ones(5, dtype=torch.int64)) is None
    for dt in (torch.float32, torch.float64):
        assert ops.prior_grid_span(dt) * torch.empty((), dtype=dt).element_size() == ops.PRIOR_MAX_BLOCKS * 256 * 32
    with pytest.raises(ValueError):
        ops.prior_eval('laplace', x, mean=0.0, scale=1.0)


def test_bad_arguments_are_rejected_without_launching():
    """every call here is refused before a launch: the pointers are dummies that are never dereferenced"""
    from bayeslim_amd._lib import lib
    one, big = ctypes.c_void_p(8), 1 << 20
    assert lib.rime_prior_workspace() == 2048 * 8

    def fwd(dtype=0, kind=0, side=0, x=one, N=12, m=(one, 1), s=(one, 1), l=(None, 0), u=(None, 0), c=(None, 0), out=one,
            ws=one, nws=big):
        return lib.rime_prior_fwd(dtype, kind, side, x, N, *m, *s, *l, *u, *c, out, None, ws, nws, None)

    assert fwd(x=None) == -1 and fwd(out=None) == -1 and fwd(N=0) == -1
    assert fwd(dtype=2) == -1 and fwd(kind=3) == -1 and fwd(kind=-1) == -1 and fwd(side=3) == -1 and fwd(side=-1) == -1
    assert fwd(m=(one, 0)) == -1 and fwd(s=(one, 13)) == -1                       # a period of 0, above N
    assert fwd(m=(one, 5)) == -1 and fwd(s=(one, 8)) == -1                        # between 1 and N, not dividing N
    assert fwd(m=(None, 0)) == -1 and fwd(s=(None, 0)) == -1                      # laplace without mean / scale
    for kind in (1, 2):
        assert fwd(kind=kind, l=(None, 0), u=(None, 0), c=(one, 1)) == -1         # a taper without bounds
        assert fwd(kind=kind, l=(one, 1), u=(one, 1), c=(None, 0)) == -1          # ... without its coefficient
        assert fwd(kind=kind, l=(one, 7), c=(one, 1)) == -1
        assert fwd(kind=kind, l=(one, 4), u=(one, 12), c=(one, 3), nws=8) == -2   # valid but for the workspace
    assert fwd(m=(one, 6), s=(one, 12), nws=2048 * 8 - 1) == -2 and fwd(ws=None) == -2
    assert lib.rime_prior_bwd(0, None, one, 12, one, None) == -1 and lib.rime_prior_bwd(0, one, None, 12, one, None) == -1
    assert lib.rime_prior_bwd(0, one, one, 12, None, None) == -1 and lib.rime_prior_bwd(0, one, one, 0, one, None) == -1
    assert lib.rime_prior_bwd(3, one, one, 12, one, None) == -1


def test_prior_kernels_use_no_scratch():
    asm, kernels, sizes = kernel_asm.read('prior')
    assert len(kernels) == 10 and len(sizes) == 10 and max(sizes) == 0, (kernels, sizes)
    assert sum('prior_fwd_kernel' in k for k in kernels) == 6 and 'scratch_' not in asm
    assert 'global_atomic' not in asm
