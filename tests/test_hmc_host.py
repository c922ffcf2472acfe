"""
CPU-side checks of the sampler layer (bayeslim_amd/paramdict.py, bayeslim_amd/sampler.py, rime_hmc_step): ParamDict on its
own, the numpy restatement of tests/hmc_common.py against the reference's recorded results (tests/golden/hmc.npz) with its
decisions, argument validation of the two entry points without a GPU, the workspace size, what the sampler refuses, the chain
files, and the no-scratch property of the built kernels.
"""
import ctypes

import numpy as np
import pytest
import torch

import hmc_common as hc
import kernel_asm


def pdict(seed=0, dtype=torch.float64):
    from bayeslim_amd.paramdict import ParamDict
    g = torch.Generator().manual_seed(seed)
    return ParamDict({'a': torch.rand(3, 4, generator=g, dtype=dtype) + 0.5, 'b': torch.rand(5, generator=g, dtype=dtype) + 0.5})


def same(x, y):
    return x.keys() == y.keys() and all(torch.equal(x[k], y[k]) for k in x)


# ------------------------------------------------------------------------------------------------------------------ ParamDict
def test_paramdict_is_a_dictionary_of_tensors():
    x = pdict()
    assert x.keys() == ['a', 'b'] and list(x) == ['a', 'b'] and len(x.values()) == 2 and x.items()[1][0] == 'b'
    assert x['a'].shape == (3, 4) and x.devices['a'] == torch.device('cpu')
    x['c'] = torch.zeros(2)
    assert x.keys() == ['a', 'b', 'c']
    y = pdict(1)
    x.update(y)
    assert same(pdict(1), type(x)({k: x[k] for k in ('a', 'b')})) and x.devices['c'] == torch.device('cpu')


def test_paramdict_arithmetic_against_a_scalar_a_tensor_and_a_paramdict():
    x, y = pdict(0), pdict(1)
    t = torch.tensor(1.5, dtype=torch.float64)
    ops = [(lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: a * b), (lambda a, b: a / b),
           (lambda a, b: b + a), (lambda a, b: b - a), (lambda a, b: b * a), (lambda a, b: b / a)]
    for f in ops:
        for other in (2.0, t, y):
            got = f(x, other)
            for k in x:
                assert torch.equal(got[k], f(x[k], other[k] if other is y else other)), k
    assert same(-x, x * -1.0) and same(x ** 2, x * x) and same(x ** 0.5, x.operator(torch.sqrt))
    # the matrix product, from both sides
    m = {'a': torch.ones(4, 2, dtype=torch.float64), 'b': torch.ones(5, dtype=torch.float64)}
    from bayeslim_amd.paramdict import ParamDict
    got = x @ ParamDict(m)
    assert torch.equal(got['a'], x['a'] @ m['a']) and torch.equal(got['b'], x['b'] @ m['b'])
    got = torch.ones(5, dtype=torch.float64) @ ParamDict({'b': x['b']})
    assert torch.equal(got['b'], torch.ones(5, dtype=torch.float64) @ x['b'])
    # in place: the tensors themselves change
    z = x.clone()
    held = z['a']
    z += y
    z *= 2.0
    z -= t
    z /= y
    assert held is z['a'] and same(z, ((x + y) * 2.0 - t) / y)
    sq = ParamDict({'a': torch.eye(3, dtype=torch.float64) * 2})
    sq @= ParamDict({'a': torch.eye(3, dtype=torch.float64) * 3})
    assert torch.equal(sq['a'], torch.eye(3, dtype=torch.float64) * 6)


def test_paramdict_operator_push_copy_clone():
    from bayeslim_amd.paramdict import ParamDict
    x, y = pdict(0), pdict(1)
    got = x.operator(lambda a, b, s: a * b + s, args=(y, 3.0))
    assert same(got, x * y + 3.0)
    z = x.clone()
    assert z.operator(torch.log, inplace=True) is None and same(z, x.operator(torch.log))
    assert same(x.operator(lambda a, d: a + d, args=({'a': 1.0, 'b': 2.0},)), ParamDict({'a': x['a'] + 1, 'b': x['b'] + 2}))
    # push: a dtype in place, a copy otherwise
    w = x.push(torch.float32, inplace=False)
    assert w['a'].dtype == torch.float32 and x['a'].dtype == torch.float64
    x2 = x.clone()
    assert x2.push(torch.float32) is None and x2['b'].dtype == torch.float32
    assert x.push({'a': 'cpu', 'b': 'cpu'}, inplace=False, copy=False).devices == x.devices
    # copy and clone are independent of their source; copy keeps Parameter-ness, clone stays in the graph, detach shares
    p = ParamDict({'a': torch.nn.Parameter(torch.ones(3)), 'b': torch.ones(2)})
    c, cl, d = p.copy(), p.clone(), p.detach()
    assert isinstance(c['a'], torch.nn.Parameter) and c['a'].is_leaf and not isinstance(c['b'], torch.nn.Parameter)
    assert cl['a'].grad_fn is not None and not d['a'].requires_grad and d['a'].data_ptr() == p['a'].data_ptr()
    with torch.no_grad():
        c['a'] += 1
        cl['b'] += 1
    assert torch.equal(p['a'].detach(), torch.ones(3)) and torch.equal(p['b'], torch.ones(2))
    o = x.ones()
    assert all(bool((o[k] == 1).all()) for k in o) and not bool((x['a'] == 1).all())


def test_paramdict_pickle_round_trip_and_model2pdict(tmp_path):
    from bayeslim_amd.paramdict import ParamDict, model2pdict
    from bayeslim_amd import utils
    x = pdict(3)
    f = str(tmp_path / 'x.pkl')
    x.write_pkl(f)
    assert same(ParamDict.read_pkl(f), x) and same(ParamDict.read_pkl(f, force_cpu=True), x)
    (x * 2).write_pkl(f)                                 # kept: no overwrite
    assert same(ParamDict.read_pkl(f), x)
    (x * 2).write_pkl(f, overwrite=True)
    assert same(ParamDict.read_pkl(f), x * 2)

    class Leaf(utils.Module):
        def __init__(self, n, grad):
            super().__init__()
            self.params = torch.nn.Parameter(torch.ones(n)) if grad else torch.ones(n)

    top = utils.Module()
    top.sky, top.beam = Leaf(2, True), Leaf(3, False)
    assert model2pdict(top).keys() == ['sky.params'] and model2pdict(top)['sky.params'] is top.sky.params
    allp = model2pdict(top, parameters=False, clone=True, prefix='m.')
    assert allp.keys() == ['m.sky.params', 'm.beam.params'] and allp['m.sky.params'] is not top.sky.params


# ---------------------------------------------------------------------------------------- the restatement against the record
def leap_grad(a, tensor_key=None):
    def grad(q):
        if tensor_key is not None:
            return hc.grad_U(a[tensor_key], q)
        return hc.chain_potential(a)(q)
    return grad


@pytest.mark.parametrize('name', list(hc.LEAP_CASES))
def test_restated_leapfrog_reproduces_the_reference(name):
    g = hc.golden()
    cont, keys, q0, p0, a, eps, cov = hc.leap_inputs(g, name)
    states = [] if name == hc.LEAP_STATES else None
    if cont == 'tensor':
        k = keys[0]
        q, p, _ = hc.oracle_leapfrog(q0[k], p0[k], leap_grad(a, k), eps if isinstance(eps, float) else eps[k], hc.LEAP_N,
                                     None if cov is None else cov[k])
        q, p = {k: q}, {k: p}
    else:
        q, p, _ = hc.oracle_leapfrog(q0, p0, leap_grad(a), eps, hc.LEAP_N, cov, states=states)
    worst = 0.0
    for k in keys:
        for got, what in ((q[k], 'q'), (p[k], 'p')):
            ref = g['leap_%s_%s_%s' % (name, what, k)]
            assert got.shape == ref.shape and got.dtype == ref.dtype
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
        if states is not None:
            assert len(states) == hc.LEAP_N + 1
            for i, what in ((0, 'q'), (1, 'p')):
                ref = g['leap_%s_states_%s_%s' % (name, what, k)]
                worst = max(worst, float(np.abs(np.stack([s[i][k] for s in states]) - ref).max() / np.abs(ref).max()))
    print('leapfrog %s: %.3e' % (name, worst))
    assert worst <= hc.FACTOR * hc.LEAP_RESTATEMENT
    # not vacuous: the trajectory moved by far more than the tolerance
    assert all(float(np.abs(q[k] - q0[k]).max()) > 1e-3 for k in keys)


@pytest.mark.parametrize('tag', ['b', 'c'])
def test_restated_chain_reproduces_the_reference_and_its_decisions(tag):
    g = hc.golden()
    recs = hc.run_oracle_chain(g, tag)
    e = hc.chain_discrepancy(recs, g, tag)                         # asserts equal accept / divergence decisions
    print('chain %s: %.3e' % (tag, e))
    assert e <= hc.FACTOR * hc.CHAIN_RESTATEMENT
    # the uniform draws are the recorded ones (a seeded host generator reproduces the reference's decisions)
    u, ref = np.array([r['u'] for r in recs]), g['chain_%s_u' % tag]
    assert np.array_equal(np.isnan(u), np.isnan(ref)) and np.array_equal(u[~np.isnan(u)], ref[~np.isnan(ref)])
    # and the record is robust: margins as the generator asserted them
    ok = ~g['chain_%s_div' % tag].astype(bool)
    assert np.all(np.abs(ref[ok] - g['chain_%s_prob' % tag][ok]) > hc.MARGIN)
    dH = g['chain_%s_H_end' % tag] - g['chain_%s_H_start' % tag]
    assert np.all(np.abs(dH - hc.CHAIN['dHmax_' + tag]) > hc.MARGIN)
    acc = g['chain_%s_accept' % tag].astype(bool)
    if tag == 'b':
        assert acc.any() and not acc.all() and not (~ok).any()
    else:
        assert (~ok).any() and ok.any()


def test_restated_dual_averaging_reproduces_the_reference():
    g = hc.golden()
    a, x0, cov, hess, draws = hc.chain_inputs(g)
    np.random.seed(hc.CHAIN['seed'])
    h = hc.OracleHMC(a, x0, hc.dual_eps0(), cov, hess, hc.CHAIN['Nstep'], hc.CHAIN['dHmax_b'], draws)
    h.dual_averaging(hc.CHAIN['Nadapt'])
    worst = max(abs(h.eps[k] - float(g['dual_eps_' + k])) / float(g['dual_eps_' + k]) for k in hc.CHAIN['keys'])
    print('dual averaging: %.3e' % worst)
    assert worst <= hc.FACTOR * hc.CHAIN_RESTATEMENT
    assert all(abs(h.eps[k] / hc.dual_eps0()[k] - 1) > 0.5 for k in h.eps)           # it adapted


def test_oracle_step_is_the_documented_arithmetic():
    """the long double restatement of one launch against exact rational arithmetic on a handful of elements, and the
    bounds' zero rule"""
    from fractions import Fraction as F
    rng = np.random.default_rng(3)
    n = 7
    q, p, g, eps, c = [rng.normal(size=n).astype(np.float32) for _ in range(5)]
    q1, p1, E1 = hc.oracle_step(q, p, g, eps, c, 0.3, 0.7, np.float32)
    k, d = F(float(np.float32(0.3))), F(float(np.float32(0.7)))
    E = F(0)
    frac = lambda x: F(float(x)) + F(float(x - np.longdouble(float(x))))          # a long double exactly, in two halves
    for i in range(n):
        pe = F(float(p[i])) - k * F(float(eps[i])) * F(float(g[i]))
        qe = F(float(q[i])) + d * F(float(eps[i])) * F(float(c[i])) ** 2 * pe
        E += (F(float(c[i])) * pe) ** 2 / 2
        assert abs(float(frac(p1[i]) - pe)) <= 4 * hc.UO * (abs(float(p[i])) + abs(float(pe))) + 1e-30
        assert abs(float(frac(q1[i]) - qe)) <= 8 * hc.UO * (abs(float(q[i])) + abs(float(qe))) + 1e-30
    assert abs(float(E1) - float(E)) <= 1e-15 * float(E)
    # every flag and null combination keeps its meaning
    q2, p2, E2 = hc.oracle_step(q, p, None, None, None, 0.0, 0.7, np.float64)
    assert np.array_equal(p2, p.astype(np.longdouble)) and np.array_equal(q2, q.astype(np.longdouble) + np.longdouble(0.7) * p)
    assert abs(float(E2) - float((p.astype(np.float64) ** 2).sum() / 2)) <= 1e-15 * float(E2)
    q3, p3, _ = hc.oracle_step(q, p, g, None, c, 0.3, 0.0, np.float64)
    assert np.array_equal(q3, q.astype(np.longdouble)) and not np.array_equal(p3, p.astype(np.longdouble))
    z = np.zeros(3, dtype=np.float32)
    assert hc.ratio(z, hc.p_bound(z, z, None, 0.5, np.float32)) == 0.0
    assert hc.ratio(np.array([0.0, 1e-30, 0.0]), hc.p_bound(z, z, None, 0.5, np.float32)) == float('inf')


# ---------------------------------------------------------------------------------------------------------- the entry points
def test_entry_points_reject_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)      # non-null dummy; never dereferenced on a rejected call
    big = 1 << 20

    def step(dtype=0, N=100, q=one, p=one, g=one, eps=None, c=None, kick=0.5, drift=1.0, energy=None, ws=one, nbytes=big):
        return lib.rime_hmc_step(dtype, N, q, p, g, eps, c, kick, drift, energy, ws, nbytes, None)

    assert step(dtype=2) == -1 and step(dtype=-1) == -1                          # unknown dtype
    assert step(N=-1) == -1 and step(N=-(1 << 40)) == -1
    assert step(p=None) == -1
    assert step(g=None) == -1 and step(q=None) == -1                            # needed by a non-zero flag
    assert step(kick=float('nan')) == -1 and step(drift=float('nan')) == -1
    assert step(kick=1e-60) == -1 and step(dtype=1, kick=1e-60, g=None) == -1    # rounds to zero in float32; float64: g needed
    need = lib.rime_hmc_workspace(100)
    assert need > 0
    assert step(energy=one, nbytes=need - 1) == -2 and step(energy=one, ws=None) == -2
    assert step(kick=0.0, drift=0.0, g=None, q=None, energy=one, nbytes=0) == -2   # the energy-only pass needs it too
    assert step(energy=one, N=-1, nbytes=0) == -1                                # the arguments are judged before the workspace
    assert step(kick=0.0, drift=0.0, g=None, q=None) == 0                        # nothing asked: nothing launched
    assert lib.rime_hmc_workspace(-1) == 0


def test_workspace_is_monotone():
    from bayeslim_amd._lib import lib
    from bayeslim_amd import sampler
    w = lib.rime_hmc_workspace
    Ns = [0, 1, 63, 2048, 2049, 4096, 4097, 10 ** 5, 10 ** 7, 5 * 10 ** 7, 10 ** 10]
    sizes = [w(N) for N in Ns]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] == 8 and sizes[1] == 8
    # one partial per work-group of the float64 span, at most STEP_MAXBLOCKS of them
    assert w(sampler.STEP_SPAN[torch.float64] + 1) == 16 and w(10 ** 10) == sampler.STEP_MAXBLOCKS * 8


# ------------------------------------------------------------------------------------------------------- what the sampler refuses
def test_sampler_names_what_it_does_not_provide_and_has_no_cpu_path():
    import bayeslim_amd
    from bayeslim_amd import sampler
    from bayeslim_amd.paramdict import ParamDict
    assert bayeslim_amd.sampler is sampler and bayeslim_amd.paramdict.ParamDict is ParamDict
    x = ParamDict({'a': torch.zeros(4, 3), 'b': torch.zeros(5)})
    pot = lambda x: (torch.tensor(0.0), x * 0)
    eye = ParamDict({'a': torch.eye(12), 'b': torch.eye(5)})

    def refuses(match, **kw):
        with pytest.raises(NotImplementedError, match=match):
            sampler.HMC(pot, x, 0.1, **kw)

    refuses('diag_mass=False', diag_mass=False)
    refuses('diag_mass=False', diag_mass={'a': True, 'b': False})
    refuses('hmat', cov_L=eye)                                   # a dense factor
    refuses('hmat', hess_L=eye)
    refuses('hmat', cov_L={'a': object(), 'b': None})            # an operator object (SolveMat, HierMat, ...)
    refuses('hmat', hess_L=torch.eye(5))
    refuses('pmask', pmask={'a': torch.ones(4, 3), 'b': torch.ones(5)})
    with pytest.raises(NotImplementedError, match='StepSize'):
        sampler.HMC(pot, x, ParamDict({'a': torch.ones(4, 3, dtype=torch.complex64), 'b': torch.ones(5)}))
    for cls, word in ((sampler.RecycledHMC, 'RecycledHMC'), (sampler.NUTS, 'NUTS'), (sampler.TreeInfo, 'TreeInfo'),
                      (sampler.StepSize, 'StepSize'), (sampler.DynamicStepSize, 'DynamicStepSize')):
        with pytest.raises(NotImplementedError, match=word):
            cls(pot, x, 0.1)
    with pytest.raises(NotImplementedError, match='estimate_cov'):
        sampler.HMC.estimate_cov(None)
    for word in ('diag_mass=False', 'pmask', 'RecycledHMC', 'NUTS', 'TreeInfo', 'StepSize', 'DynamicStepSize', 'estimate_cov'):
        assert word in sampler.__doc__, word
    # CPU tensors: the project's error, from the sampler, from leapfrog and from one launch
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        sampler.HMC(pot, x, 0.1)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        sampler.leapfrog(torch.zeros(5), torch.zeros(5), lambda q, Ucache=None: q, 0.1, 3)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        sampler.leapfrog(x.clone(), x.clone(), lambda q, Ucache=None: q, 0.1, 3)
    with pytest.raises(NotImplementedError, match='diag_mass=False'):
        sampler.leapfrog(torch.zeros(5), torch.zeros(5), lambda q, Ucache=None: q, 0.1, 3, cov_L=torch.eye(5), diag_mass=False)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        sampler.hmc_step(torch.zeros(5), torch.zeros(5), torch.zeros(5), None, None, 0.5, 1.0)


def test_uturn_and_chain_files(tmp_path):
    from bayeslim_amd import sampler
    from bayeslim_amd.paramdict import ParamDict
    one = torch.ones(3, dtype=torch.float64)
    assert not sampler.hoffman_uturn(0 * one, one, one, one)
    assert sampler.hoffman_uturn(0 * one, one, -one, one) and sampler.hoffman_uturn(0 * one, one, one, -one)
    z = torch.tensor([1j, 1.0])
    assert not sampler.hoffman_uturn(ParamDict({'k': 0 * z}), ParamDict({'k': z}), ParamDict({'k': z}), ParamDict({'k': z}))
    assert sampler.hoffman_uturn(ParamDict({'k': 0 * z}), ParamDict({'k': z}), ParamDict({'k': -z}), ParamDict({'k': z}))

    x0 = ParamDict({'a': torch.arange(6.0).reshape(2, 3), 'b': torch.ones(4)})
    s = sampler.SamplerBase(x0)
    assert s.x['a'] is not x0['a'] and s.accept_ratio == 1.0 and s.chain == {'a': [], 'b': []}
    with pytest.raises(NotImplementedError):
        s.step()
    for i in range(4):
        s.x = x0 * float(i)
        s.append_chain(s.x, U=10.0 + i)
        s._acceptances.append(np.asarray(i % 2 == 0))
    f = str(tmp_path / 'chain.npz')
    s.write_chain(f, description='four entries')
    assert s.accept_ratio == 0.5
    t = sampler.SamplerBase(x0)
    t.load_chain(f)
    assert t.Uchain == [10.0, 11.0, 12.0, 13.0] and t.accept_ratio == 0.5 and len(t._acceptances) == 4
    assert all(np.array_equal(np.asarray(t.chain[k]), np.asarray(s.chain[k])) for k in ('a', 'b'))
    assert torch.equal(t.x['a'], s.x['a']) and t.get_chain('a')['a'].shape == (4, 2, 3)
    assert set(t.get_chain()) == {'a', 'b'}
    s.Uchain[0] = -1.0
    s.write_chain(f)                                             # kept: no overwrite
    t.load_chain(f)
    assert t.Uchain[0] == 10.0
    s.write_chain(f, overwrite=True)
    t.load_chain(f)
    assert t.Uchain[0] == -1.0
    t.clear_chain(3)
    assert t.Uchain == [13.0] and len(t.chain['a']) == 1
    t.clear_chain()
    assert t.Uchain == [] and t.chain == {'a': [], 'b': []}


def test_hmc_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/hmc.hip: no kernel has a private segment"""
    _, kernels, sizes = kernel_asm.read('hmc')
    # the stage in 2 precisions + the second reduction stage
    assert len(kernels) == 3 and all('hmc_' in k for k in kernels), kernels
    assert len(sizes) == 3 and max(sizes) == 0, sizes
