"""
CPU-side checks of bayeslim_amd/recycled.py and rime_hmc_recycle: the export and its signature, every host-side refusal of the entry
point (they return before any HIP call), the no-scratch property of the built kernels, StepSize / DynamicStepSize / multiply_eps /
estimate_cov against their defining equations, what the constructors refuse, that the stubs of sampler.py still refuse, and on the
golden file that the restatement of tests/recycled_common.py reproduces the reference's chains and that every recorded margin
exceeds the float32 bound.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hmc_common as hc
import kernel_asm
import recycled_common as rc
from bayeslim_amd import _lib, recycled, sampler
from bayeslim_amd.paramdict import ParamDict

EINVAL, EWORKSPACE = -1, -2
PTR = lambda k: ctypes.c_void_p(4096 * (k + 1))           # distinct non-null dummies 4096 bytes apart; never dereferenced


# ---------------------------------------------------------------------------------------------------------- the entry point
def test_library_header_and_binding_agree():
    assert hasattr(_lib.lib, 'rime_hmc_recycle')
    res, args = _lib.SIGNATURES['rime_hmc_recycle']
    header = open(os.path.join(kernel_asm.ROOT, 'include', 'rime_hip.h')).read()
    m = re.search(r'int rime_hmc_recycle\(([^;]*)\);', header)
    assert m is not None and res is ctypes.c_int
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    kind = lambda p: (ctypes.c_void_p if '*' in p else {'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'double': ctypes.c_double,
                                                       'size_t': ctypes.c_size_t}[p.rsplit(' ', 1)[0]])
    assert [kind(p) for p in params] == args
    assert [p.rsplit(' ', 1)[1].lstrip('*') for p in params] == ['dtype', 'N', 'q', 'p', 'g', 'eps', 'c', 'half', 'drift', 'q_out',
                                                                'p_out', 'energy', 'workspace', 'workspace_bytes', 'stream']
    mk = open(os.path.join(kernel_asm.ROOT, 'bayeslim_amd', 'csrc', 'Makefile')).read()
    assert 'recycle.hip' in mk and re.search(r'ASM_SRCS = .*\brecycle\b', mk)


def _recycle(**bad):
    a = dict(dtype=0, N=100, q=PTR(0), p=PTR(1), g=PTR(2), eps=None, c=None, half=0.5, drift=1.0, q_out=PTR(3), p_out=PTR(4),
             energy=PTR(5), workspace=PTR(6), workspace_bytes=_lib.lib.rime_hmc_workspace(100), stream=None)
    a.update(bad)
    return _lib.lib.rime_hmc_recycle(*a.values())


@pytest.mark.parametrize('bad,code', [
    (dict(dtype=2), EINVAL), (dict(dtype=-1), EINVAL), (dict(N=-1), EINVAL), (dict(N=0x3fffffffffffffff + 1), EINVAL),
    (dict(p=None), EINVAL), (dict(q=None), EINVAL), (dict(g=None), EINVAL), (dict(q_out=None), EINVAL), (dict(p_out=None), EINVAL),
    (dict(energy=None), EINVAL), (dict(half=float('nan')), EINVAL), (dict(drift=float('nan')), EINVAL), (dict(half=0.0), EINVAL),
    (dict(half=1e-60), EINVAL), (dict(drift=1e-60), EINVAL), (dict(drift=-1e-60), EINVAL),
    (dict(workspace=None), EWORKSPACE), (dict(workspace_bytes=7), EWORKSPACE), (dict(N=512, dtype=1, workspace_bytes=0), EWORKSPACE),
    (dict(half=1e-60, workspace=None), EWORKSPACE),                                  # looked at before the rounding
    (dict(N=-1, workspace=None), EINVAL),                                            # the arguments are judged first
    (dict(q_out=PTR(0)), EINVAL), (dict(q_out=PTR(1)), EINVAL), (dict(q_out=PTR(2)), EINVAL),
    (dict(p_out=PTR(0)), EINVAL), (dict(p_out=PTR(1)), EINVAL), (dict(p_out=PTR(2)), EINVAL), (dict(p_out=PTR(3)), EINVAL),
    (dict(q_out=ctypes.c_void_p(4096 * 2 - 4)), EINVAL),                             # on the first element of p
    (dict(eps=PTR(7), q_out=PTR(7)), EINVAL), (dict(eps=PTR(7), p_out=PTR(7)), EINVAL),  # the optional vectors, when given
    (dict(c=PTR(7), q_out=PTR(7)), EINVAL), (dict(c=PTR(7), p_out=ctypes.c_void_p(4096 * 8 + 396)), EINVAL),
    (dict(p_out=ctypes.c_void_p(4096 * 3 + 396)), EINVAL),                           # on the last element of g
], ids=lambda b: '-'.join(b) if isinstance(b, dict) else str(b))
def test_entry_point_rejects_without_launching(bad, code):
    assert _recycle(**bad) == code


def test_overlap_is_judged_in_the_working_type():
    """float64 vectors of 100 elements are 800 bytes: a base 400 bytes into another overlaps, in float32 it touches its end"""
    assert _recycle(dtype=1, q_out=ctypes.c_void_p(4096 + 400 + 396)) == EINVAL
    assert _recycle(dtype=1, q_out=ctypes.c_void_p(4096 - 796)) == EINVAL


def test_recycle_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/recycle.hip: no kernel has a private segment, none an atomic"""
    asm, kernels, sizes = kernel_asm.read('recycle')
    # the stage in 2 precisions + the second reduction stage
    assert len(kernels) == 3 and all('hmc_recycle' in k for k in kernels), kernels
    assert len(sizes) == 3 and max(sizes) == 0, sizes
    assert 'scratch_load' not in asm and 'scratch_store' not in asm and 'global_atomic' not in asm


# ---------------------------------------------------------------------------------------------------------- step sizes
def _eps():
    return {'a': torch.tensor([1 + 2j, 3 + 4j], dtype=torch.complex128), 'b': torch.tensor([0.5, 0.25], dtype=torch.float64)}


def _x():
    return ParamDict({'a': torch.tensor([1 + 1j, 2 - 1j], dtype=torch.complex128), 'b': torch.tensor([2.0, 4.0], dtype=torch.float64)})


def test_multiply_eps():
    x, e = _x(), _eps()
    assert torch.equal(recycled.multiply_eps(x['a'], e['a']), torch.complex(x['a'].real * e['a'].real, x['a'].imag * e['a'].imag))
    assert torch.equal(recycled.multiply_eps(x['a'], e['a']), torch.tensor([1 + 2j, 6 - 4j], dtype=torch.complex128))
    assert torch.equal(recycled.multiply_eps(x['b'], e['b']), x['b'] * e['b'])
    assert torch.equal(recycled.multiply_eps(x['a'], e['b']), x['a'] * e['b'])          # a real step of a complex tensor
    assert torch.equal(recycled.multiply_eps(x['b'], 0.5), x['b'] * 0.5)
    with pytest.raises(ValueError, match='complex'):
        recycled.multiply_eps(x['b'], e['a'])


def test_stepsize_arithmetic():
    x, e = _x(), recycled.StepSize(_eps())
    raw = _eps()
    assert isinstance(e, ParamDict) and e.is_complex == {'a': True, 'b': False} and e.keys() == ['a', 'b']
    got = e * x
    assert got.__class__ is ParamDict and all(torch.equal(got[k], recycled.multiply_eps(x[k], raw[k])) for k in raw)
    got = x * e                                                  # the ParamDict's own, plain product
    assert got.__class__ is ParamDict and all(torch.equal(got[k], x[k] * raw[k]) for k in raw)
    for f in ((lambda a, b: a / b), (lambda a, b: a + b), (lambda a, b: a - b), (lambda a, b: b / a), (lambda a, b: b - a),
              (lambda a, b: b + a)):
        for other in (2.0, {'a': 2.0, 'b': 4.0}):
            got = f(e, other)
            assert isinstance(got, recycled.StepSize)
            assert all(torch.equal(got[k], f(raw[k], other[k] if isinstance(other, dict) else other)) for k in raw), (got, other)
    assert all(torch.equal((e ** 2)[k], raw[k] ** 2) for k in raw)
    half = e / 2
    assert torch.equal(half['a'], raw['a'] / 2) and torch.equal(e['a'], raw['a'])       # a new object: e is unchanged
    prod = e * recycled.StepSize({'a': raw['a'], 'b': raw['b']})
    assert isinstance(prod, recycled.StepSize) and torch.equal(prod['a'], recycled.multiply_eps(raw['a'], raw['a']))
    c = e.copy()
    assert c is not e and c['a'] is e['a']                                              # shallow
    held = c['b']
    c = recycled.StepSize({k: v.clone() for k, v in raw.items()})
    held = c['b']
    c += 1.0
    c -= {'a': 1.0, 'b': 0.5}
    c /= 2.0
    c *= 2.0
    assert c['b'] is held and torch.equal(c['b'], ((raw['b'] + 1.0 - 0.5) / 2.0) * 2.0)
    c.push(torch.float32)
    assert c['b'].dtype == torch.float32 and c['a'].dtype == torch.complex64
    assert e.values()[1] is e['b'] and e.items()[0][0] == 'a' and 'StepSize' in repr(e)


def test_dynamic_stepsize():
    p = {'a': torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), 'b': torch.tensor([4.0], dtype=torch.float64)}
    d = recycled.DynamicStepSize(p, gamma=0.5, min_prob=0.3, alpha=1.5, track=True)
    assert all(float(v) == 1.0 for v in d.eps_mul.values()) and d.chain == []
    d.update(0.1)
    d.update(torch.tensor(0.2))
    assert float(d.eps_mul['a']) == 0.25 and torch.equal(d['a'], p['a'] * 0.25) and torch.equal(d['b'], p['b'] * 0.25)
    d.update(0.3)                                                # not below min_prob: grows by alpha
    assert float(d.eps_mul['a']) == 0.375
    d.update(0.9), d.update(0.9), d.update(0.9)
    assert float(d.eps_mul['a']) == 1.0                          # 0.5625, 0.84375, then capped
    assert [float(c['a']) for c in d.chain] == [1.0, 0.5, 0.25, 0.375, 0.5625, 0.84375]
    # an index: only those elements follow the multiplier
    d = recycled.DynamicStepSize(p, gamma=0.5, index={'a': slice(0, 2), 'b': torch.tensor([0])})
    d.update(0.0)
    assert torch.equal(d['a'], torch.tensor([0.5, 1.0, 3.0], dtype=torch.float64)) and torch.equal(d['b'], p['b'] * 0.5)
    assert torch.equal(p['a'], torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)) and d.chain is None
    # arithmetic acts on params and keeps eps_mul; the reflected forms return the effective step with the multiplier reset
    h = d / 2
    assert isinstance(h, recycled.DynamicStepSize) and torch.equal(h.params['a'], p['a'] / 2) and float(h.eps_mul['a']) == 0.5
    assert h.gamma == 0.5 and h.index is d.index
    r = 1.0 / d
    assert float(r.eps_mul['a']) == 1.0 and torch.equal(r.params['a'], 1.0 / d['a'])
    c = d.copy(track=True, chain=[1])
    assert c.chain == [1] and c.params is d.params and c.min_prob == d.min_prob and c.alpha == d.alpha
    x = ParamDict({'a': torch.ones(3, dtype=torch.float64), 'b': torch.ones(1, dtype=torch.float64)})
    assert torch.equal((d * x)['a'], d['a'])
    with pytest.raises(TypeError):
        recycled.DynamicStepSize(p, eps_mul=1.0)


def test_expand_eps_layout():
    f = torch.float64
    lay = sampler._Layout(ParamDict({'u': torch.zeros(3, dtype=f), 'w': torch.zeros(2, dtype=torch.complex128), 'v': torch.zeros(2, dtype=f)}))
    w = torch.tensor([1 + 2j, 3 + 4j], dtype=torch.complex128)
    flat = recycled.expand_eps(lay, {'u': 0.5, 'w': w, 'v': torch.tensor([7.0, 8.0], dtype=f)})
    assert flat.tolist() == [0.5, 0.5, 0.5, 1.0, 1.0, 2.0, 3.0, 4.0, 7.0, 8.0]          # the gap at element 3 holds one
    assert recycled.expand_eps(lay, {'u': 0.5, 'w': torch.tensor(1 + 2j), 'v': None}).tolist() == [0.5] * 3 + [1.0] + [1.0, 2.0] * 2 + [1.0] * 2
    assert recycled.expand_eps(lay, recycled.StepSize({'u': torch.tensor(0.5), 'w': w, 'v': torch.tensor(2.0)})).tolist()[4:8] == [1.0, 2.0, 3.0, 4.0]
    # without complex values it is _Layout.expand itself
    assert recycled.expand_eps(lay, 0.3) == 0.3 and recycled.expand_eps(lay, None) is None
    e = {'u': torch.tensor([1.0, 2.0, 3.0], dtype=f), 'w': torch.tensor([4.0, 5.0], dtype=f), 'v': 0.5}
    assert torch.equal(recycled.expand_eps(lay, e), lay.expand(e, 'eps'))
    d = recycled.DynamicStepSize({'u': torch.ones(3, dtype=f), 'w': torch.ones(2, dtype=f), 'v': torch.ones(2, dtype=f)}, gamma=0.5)
    d.update(0.0)
    assert recycled.expand_eps(lay, d).tolist() == [0.5] * 3 + [1.0] + [0.5] * 6
    with pytest.raises(ValueError, match='real parameter'):
        recycled.expand_eps(lay, {'u': torch.ones(3, dtype=torch.complex128), 'w': w, 'v': 1.0})
    with pytest.raises(ValueError, match='broadcast'):
        recycled.expand_eps(lay, {'u': 1.0, 'w': torch.ones(3, dtype=torch.complex128), 'v': 1.0})
    with pytest.raises(NotImplementedError):                     # the other keys are judged in sampler's words
        recycled.expand_eps(lay, {'u': torch.ones(4, dtype=f), 'w': w, 'v': 1.0})
    with pytest.raises(NotImplementedError, match='StepSize'):   # and _Layout itself still refuses complex values
        lay.classify({'u': 1.0, 'w': w, 'v': 1.0}, 'eps')


# ---------------------------------------------------------------------------------------------------------- estimate_cov
def test_estimate_cov_against_numpy():
    rng = np.random.default_rng(5)
    chain = {'a': [rng.normal(size=(3, 5)) * np.arange(1, 6) for _ in range(40)],
             'w': [rng.normal(size=4) + 2j * rng.normal(size=4) for _ in range(40)]}
    L = recycled.estimate_cov(chain)
    assert isinstance(L, ParamDict) and L['a'].shape == (3, 5) and L['w'].shape == (4,) and L['w'].dtype == torch.float64
    assert np.array_equal(L['a'].numpy(), np.sqrt(np.var(np.array(chain['a']), axis=0)))
    assert np.array_equal(L['w'].numpy(), np.sqrt(np.var(np.array(chain['w']), axis=0)))     # real, for a complex key
    L = recycled.estimate_cov(chain, Nback=10, dtype=torch.float32)
    assert L['a'].dtype == torch.float32
    assert np.array_equal(L['a'].numpy(), np.sqrt(np.var(np.array(chain['a'])[-10:], axis=0)).astype(np.float32))
    real = {'a': chain['a']}
    x = np.array(real['a'])
    mad = 1.4826 * np.median(np.abs(x - np.median(x, axis=0)), axis=0)
    assert np.array_equal(recycled.estimate_cov(real, robust=True)['a'].numpy(), mad)
    assert np.all(np.abs(mad / np.sqrt(np.var(x, axis=0)) - 1) < 0.5)                        # it estimates the same scale
    reg = 1e-3
    Ld = recycled.estimate_cov(real, diag_mass=False, eps={'a': reg})['a'].numpy()
    cov = np.cov(x.reshape(40, -1).T)
    assert Ld.shape == (15, 15) and np.array_equal(Ld, np.tril(Ld))
    assert np.abs(Ld @ Ld.T - (cov + reg * np.eye(15))).max() <= 64 * 15 * 2.0 ** -53 * np.abs(cov).max()
    with pytest.raises(ValueError, match='real parameters'):
        recycled.estimate_cov(chain, robust=True)
    with pytest.raises(ValueError, match='real parameters'):
        recycled.estimate_cov(chain, diag_mass=False)
    with pytest.raises(ValueError, match='two or more'):
        recycled.estimate_cov({'a': chain['a'][:1]})
    assert 'undefined variable' in recycled.estimate_cov.__doc__


# ---------------------------------------------------------------------------------------------------------- what is refused
def test_constructors_judge_then_need_a_gpu():
    f = torch.float32
    x = ParamDict({'a': torch.zeros(4, 3, dtype=f), 'w': torch.zeros(5, dtype=torch.complex64)})
    pot = lambda q: (torch.tensor(0.0), q * 0)
    cw = torch.ones(5, dtype=torch.complex64)
    for cls in (recycled.HMC, recycled.RecycledHMC):
        with pytest.raises(ValueError, match='real parameter'):
            cls(pot, x, {'a': torch.ones(4, 3, dtype=torch.complex64), 'w': cw})
        with pytest.raises(ValueError, match='real parameter'):
            cls(pot, x, recycled.StepSize({'a': torch.ones(4, 3, dtype=torch.complex64), 'w': cw}))
        with pytest.raises(NotImplementedError, match='diag_mass=False'):
            cls(pot, x, 0.1, diag_mass=False)
        with pytest.raises(TypeError):
            cls(pot, {'a': torch.zeros(3)}, 0.1)
        # all arguments good: the project's error for a CPU x0, after they have been judged
        for eps in (0.1, {'a': 0.1, 'w': cw}, recycled.StepSize({'a': torch.tensor(0.1), 'w': cw}),
                    recycled.DynamicStepSize({'a': torch.full((4, 3), 0.1), 'w': cw})):
            with pytest.raises(RuntimeError, match='no CPU implementation'):
                cls(pot, x, eps)
    with pytest.raises(ValueError, match='real parameter'):
        recycled.HMC(pot, x, 0.1, pmask={'a': torch.ones(4, 3, dtype=torch.complex64), 'w': None})
    with pytest.raises(ValueError, match='broadcast'):
        recycled.HMC(pot, x, 0.1, pmask={'a': torch.ones(5), 'w': None})
    with pytest.raises(TypeError):
        recycled.HMC(pot, x, 0.1, pmask=torch.ones(3))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        recycled.HMC(pot, x, 0.1, pmask={'a': torch.ones(3), 'w': cw})
    for cls in (recycled.HMC, recycled.RecycledHMC):             # both take masks: judged, then the device
        with pytest.raises(ValueError, match='real parameter'):
            cls(pot, x, 0.1, pmask={'a': torch.ones(4, 3, dtype=torch.complex64), 'w': None})
        with pytest.raises(RuntimeError, match='no CPU implementation'):
            cls(pot, x, 0.1, pmask={'a': None, 'w': cw})
    with pytest.raises(ValueError, match='Nstep'):
        recycled.RecycledHMC(pot, x, 0.1, Nstep=0)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        recycled.hmc_recycle(*[torch.zeros(5) for _ in range(3)], None, None, 0.5, 1.0, torch.zeros(5), torch.zeros(5),
                             torch.zeros(1, dtype=torch.float64))
    # estimate_cov(diag_mass=False) on the sampler names where the dense factor lives (no instance is needed to be told)
    with pytest.raises(NotImplementedError, match=r'recycled\.estimate_cov.*massmat\.HMC\.set_chol'):
        recycled.HMC.estimate_cov(None, diag_mass=False)
    for word in ('2 * Nstep * N', 'no CPU path', 'RecycledHMC', 'StepSize', 'pmask', 'estimate_cov'):
        assert word in recycled.__doc__, word
    assert '2 * Nstep * N' in recycled.RecycledHMC.__doc__


def test_the_stubs_of_sampler_still_refuse():
    import bayeslim_amd
    assert bayeslim_amd.recycled is recycled
    x = ParamDict({'a': torch.zeros(4, 3)})
    pot = lambda q: (torch.tensor(0.0), q * 0)
    for cls, word in ((sampler.RecycledHMC, 'RecycledHMC'), (sampler.StepSize, 'StepSize'), (sampler.DynamicStepSize, 'DynamicStepSize')):
        with pytest.raises(NotImplementedError, match=word):
            cls(pot, x, 0.1)
    with pytest.raises(NotImplementedError, match='pmask'):
        sampler.HMC(pot, x, 0.1, pmask={'a': torch.ones(4, 3)})
    with pytest.raises(NotImplementedError, match='estimate_cov'):
        sampler.HMC.estimate_cov(None)
    with pytest.raises(NotImplementedError, match='StepSize'):
        sampler.HMC(pot, x, ParamDict({'a': torch.ones(4, 3, dtype=torch.complex64)}))
    assert 'bayeslim_amd.recycled' in sampler.__doc__


# ---------------------------------------------------------------------------------------------------------- the golden file
def test_oracle_recycle_is_the_composition():
    rng = np.random.default_rng(9)
    q, p, g, eps, c = [rng.normal(size=33) for _ in range(3)] + [rng.uniform(0.5, 2, 33) for _ in range(2)]
    for drift in (0.0, 0.7):
        q2, p2, qo, po, E, B = rc.oracle_recycle(q, p, g, eps, c, 0.3, drift, np.float64)
        _, p1, E1 = hc.oracle_step(q, p, g, eps, c, 0.3, 0.0, np.float64)
        assert np.array_equal(po, p1) and np.array_equal(qo, q.astype(np.longdouble)) and E == E1
        if drift:
            q3, p3, _ = hc.oracle_step(q, p1, g, eps, c, 0.3, drift, np.float64)
            assert np.array_equal(q2, q3) and np.array_equal(p2, p3) and np.all(B[1] > B[2]) and np.all(B[0] > 0)
        else:
            assert np.array_equal(p2, p1) and np.array_equal(q2, qo) and not B[0].any()


@pytest.mark.parametrize('tag', rc.TAGS)
def test_restated_chain_reproduces_the_reference_and_its_decisions(tag):
    g = rc.golden()
    recs = rc.run_oracle_chain(g, tag)
    e = rc.chain_discrepancy(recs, g, tag)                        # asserts equal accept / divergence decisions and chain lengths
    print('chain %s: %.3e' % (tag, e))
    assert e <= rc.RESTATEMENT
    assert np.array_equal(rc.padded([r['u'] for r in recs]), g[tag + '_u'], equal_nan=True)
    if tag == 'c':
        m = g['c_eps_mul']
        assert np.array_equal(rc.eps_mul_of(recs), m)
        steps = np.diff(np.vstack([np.ones((1, len(rc.KEYS))), m]), axis=0)
        assert (steps < 0).any() and (steps > 0).any()            # both branches of update
        assert set(np.log2(m).ravel()) <= {0.0, -1.0, -2.0, -3.0}  # powers of two: exact in float32 as well


@pytest.mark.parametrize('tag', rc.TAGS)
def test_recorded_chains_are_decisive_in_float32(tag):
    """every recorded margin exceeds the float32 bound on a difference of Hamiltonians, and hmc_common.MARGIN"""
    g = rc.golden()
    H, u, Hs = g[tag + '_H'], g[tag + '_u'], g[tag + '_H_start'][:, None]
    dH, ok = H - Hs, ~np.isnan(u)
    b32 = rc.dH_bound(torch.float32, float(np.nanmax(np.abs(H))))
    assert 0 < b32 < 0.05
    assert np.all(np.abs(np.log(u[ok]) - np.minimum(-dH[ok], 0.0)) > b32)
    assert np.all(np.abs(u[ok] - np.minimum(1.0, np.exp(-dH[ok]))) > hc.MARGIN)
    seen = ~np.isnan(dH)
    assert np.all(np.abs(dH[seen] - rc.CHAINS[tag]['dHmax']) > max(b32, hc.MARGIN))
    acc, div = g[tag + '_accept'], g[tag + '_div'].astype(bool)
    assert (acc[ok] == 1).any() and (acc[ok] == 0).any()
    assert (div.any() and not div.all()) if tag == 'e' else not div.any()
    assert all(v.dtype in (np.float64, np.complex128) for v in g.values()) and os.path.getsize(rc.GOLDEN) < 1 << 20
