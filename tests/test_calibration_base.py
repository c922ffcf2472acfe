"""
What the calibration terms share (calibration._CalTerm on utils.Module), tested by behaviour on CPU tensors: the chain
parameters (+ p0) -> response -> gradient hooks -> priors, push to a dtype and to a device with the caches each class clears,
the delay phasor and the baseline validation of the two setup_coupling()s, and pickling without the cached output.

The forward of every class ends on the GPU.  JonesModel, RedVisModel and VisModel run the chain before they ask for GPU
tensors, so their forward is driven on CPU tensors up to that RuntimeError; VisCoupling and RedVisCoupling ask first, so they
get an input that claims to be on the GPU and a stand-in for their `ops` call.
"""
import pickle
import types

import numpy as np
import pytest
import torch

import calterm_common as ct
from bayeslim_amd import calibration as cal


class StubResponse:
    """a response that records what it is called with and pushed to; params (..., 2) -> complex"""
    times = None
    freq_mode = time_mode = 'channel'
    param_type = 'com'

    def __init__(self):
        self.calls, self.pushed, self.out = [], [], None

    def __call__(self, params, **kwargs):
        self.calls.append(params)
        self.out = torch.view_as_complex(params) * 1
        return self.out

    def push(self, device):
        self.pushed.append(device)


class Recorder:
    """a prior (callable with push) or a gradient hook that records its arguments"""
    def __init__(self, value=None):
        self.args, self.pushed, self.value = [], [], value

    def __call__(self, x):
        self.args.append(x)
        return self.value

    def push(self, device):
        self.pushed.append(device)


class GpuLike:
    """stands for vd.data where the class asks for a GPU tensor before anything else: says it is one, holds a CPU tensor"""
    is_cuda = True

    def __init__(self, t):
        self.t, self.shape, self.dtype = t, t.shape, t.dtype

    def __getitem__(self, k):
        return self.t[k]


def forward(m, vd, name, monkeypatch, prior_cache=None):
    """one forward of the module on CPU tensors as far as it goes there"""
    if name in ('VisCoupling', 'RedVisCoupling'):
        n = m.plan.Nbl if name == 'VisCoupling' else m.plan.Nout
        fake = types.SimpleNamespace(data=GpuLike(vd.data), times=vd.times, copy=lambda **kw: types.SimpleNamespace())
        m._vd = types.SimpleNamespace()
        stand_in = lambda *a, **kw: torch.zeros(n, ct.NT, ct.NF, dtype=torch.complex128)
        monkeypatch.setattr(cal.ops, 'coupling_apply' if name == 'VisCoupling' else 'redcoupling_apply', stand_in)
        assert m(fake, prior_cache=prior_cache).data.shape == (1, 1, n, ct.NT, ct.NF)
    else:
        with pytest.raises(RuntimeError, match='needs tensors on the GPU'):
            m(vd, prior_cache=prior_cache)


def run_chain(name, monkeypatch, requires_grad=True, hooks=None):
    """a module on a stub response, run forward once; returns (module, stub response)"""
    R = StubResponse()
    m, vd = ct.build(name, R=R, p0=True)
    if not requires_grad:
        m.params.requires_grad_(False)
    m.register_response_hooks(hooks)
    forward(m, vd, name, monkeypatch)
    return m, R


@pytest.mark.parametrize('name', ct.CLASSES)
def test_p0_is_added_before_the_response(name, monkeypatch):
    m, R = run_chain(name, monkeypatch)
    assert len(R.calls) == 1
    assert m.p0 is not None and float(m.p0.abs().max()) > 0
    assert torch.equal(R.calls[0], m.params + m.p0) and not torch.equal(R.calls[0], m.params)


@pytest.mark.parametrize('name', ct.CLASSES)
def test_every_hook_is_registered_once_per_forward(name, monkeypatch):
    hooks = [Recorder(), Recorder()]
    m, R = run_chain(name, monkeypatch, hooks=hooks)
    R.out.real.sum().backward()
    assert [len(h.args) for h in hooks] == [1, 1]              # a hook registered twice would be called twice
    assert all(h.args[0].shape == R.out.shape for h in hooks)
    # nothing requires grad: no hook is registered (torch refuses a hook on such a tensor, so a try would raise)
    hooks = [Recorder(), Recorder()]
    m, R = run_chain(name, monkeypatch, requires_grad=False, hooks=hooks)
    assert not R.out.requires_grad and R.out._backward_hooks is None
    # no registry: the same forward
    run_chain(name, monkeypatch, hooks=None)


@pytest.mark.parametrize('name', ct.CLASSES)
def test_priors_get_the_parameters_and_the_response_output_once(name, monkeypatch):
    R = StubResponse()
    m, vd = ct.build(name, R=R, p0=True)
    pin, pout = Recorder(torch.tensor(2.0)), Recorder(torch.tensor(3.0))
    m.set_priors(priors_inp_params=[None, pin], priors_out_params=[pout, None])
    writes = []

    class Cache(dict):
        def __setitem__(self, k, v):
            writes.append(k)
            dict.__setitem__(self, k, v)

    cache = Cache()
    forward(m, vd, name, monkeypatch, cache)
    out = R.out
    forward(m, vd, name, monkeypatch, cache)                   # the second forward finds the key and evaluates nothing
    assert len(pin.args) == 1 and pin.args[0] is m.params
    assert len(pout.args) == 1 and pout.args[0] is out
    assert writes == [m.name] and float(cache[m.name]) == 5.0
    forward(m, vd, name, monkeypatch, None)                    # no cache: nothing to evaluate
    assert len(pin.args) == 1 and len(pout.args) == 1


# what push does, one row per class, as the classes behaved before they shared a base:
#   the floating / complex attributes a dtype push re-types; the caches a device push clears; the caches it keeps
_IDX = ('cache_tidx', 'cache_bidx')
PUSH = {
    'JonesModel': (('params', 'p0'), _IDX + ('cache_aidx', '_vd'), ()),
    'RedVisModel': (('params', 'p0'), _IDX + ('cache_plan', '_vd'), ()),
    'VisModel': (('params', 'p0'), _IDX + ('cache_plan', '_vd'), ()),
    'VisCoupling': (('params', 'p0', 'I', 'dly', 'freqs'), (), _IDX + ('_vd',)),
    'RedVisCoupling': (('params', 'p0', 'dly'), ('_vd',), _IDX),               # freqs is not pushed
}
INT_ATTRS = {'VisCoupling': ('flat_data_idx', 'flat_data_null', 'flat_conj_idx', 'flat_unconj_idx', 'bls_idx'),
             'RedVisCoupling': cal._RVC_TUPLES}


def pushed_module(name):
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)                     # setup_coupling() builds dly and I in the default precision
    try:
        m, _ = ct.build(name, R=StubResponse(), p0=True)
    finally:
        torch.set_default_dtype(old)
    priors = [Recorder(), Recorder()]
    m.set_priors(priors_inp_params=[None, priors[0]], priors_out_params=[priors[1], None])
    retyped, cleared, kept = PUSH[name]
    for k in cleared + kept:
        setattr(m, k, {'key': 'value'})
    return m, priors, retyped, cleared, kept


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('name', ct.CLASSES)
def test_push_to_a_dtype(name, dtype):
    m, priors, retyped, cleared, kept = pushed_module(name)
    was_param = isinstance(m.params, torch.nn.Parameter)
    ints = {k: getattr(m, k) for k in INT_ATTRS.get(name, ())}
    other = {k: v.dtype for k, v in vars(m).items() if torch.is_tensor(v) and k not in retyped}
    m.push(dtype)
    cdtype = torch.complex64 if dtype == torch.float32 else torch.complex128
    for k in retyped:
        v = getattr(m, k)
        assert v.dtype == (cdtype if v.is_complex() else dtype), k
    assert isinstance(m.params, torch.nn.Parameter) == was_param
    for k, dt in other.items():
        assert getattr(m, k).dtype == dt, k                    # RedVisCoupling.freqs among them
    for k, v in ints.items():                                  # index tensors keep their integer type and values
        new = getattr(m, k)
        for a, b in zip(new if isinstance(new, tuple) else (new,), v if isinstance(v, tuple) else (v,)):
            assert a.dtype == b.dtype and torch.equal(a, b)
    for k in cleared + kept:                                   # a dtype push clears no cache
        assert getattr(m, k) == {'key': 'value'}, k
    assert m.R.pushed == [dtype]
    assert [p.pushed for p in priors] == [[dtype], [dtype]]    # both lists, the None entries skipped


@pytest.mark.parametrize('name', ct.CLASSES)
def test_push_to_a_device(name):
    m, priors, retyped, cleared, kept = pushed_module(name)
    m._times = torch.arange(3.0)
    dtypes = {k: v.dtype for k, v in vars(m).items() if torch.is_tensor(v)}
    dtypes['params'] = m.params.dtype
    m.push('cpu')
    assert m.device == 'cpu' and torch.equal(m._times, torch.arange(3.0))
    for k, dt in dtypes.items():
        assert getattr(m, k).dtype == dt, k                    # a device push re-types nothing
    for k in cleared:
        assert getattr(m, k) in ({}, None), k
    for k in kept:
        assert getattr(m, k) == {'key': 'value'}, k
    assert m.R.pushed == ['cpu']
    assert [p.pushed for p in priors] == [['cpu'], ['cpu']]


@pytest.mark.parametrize('Nf', [1, 4])
@pytest.mark.parametrize('min_dly', [None, 20.0])
@pytest.mark.parametrize('sign', [1, -1])
def test_coupling_delay_is_the_two_expressions_it_replaces(sign, min_dly, Nf):
    rng = np.random.default_rng(3)
    c = 2.99792458e8
    freqs = torch.as_tensor(120e6 + 1e6 * rng.random(Nf).cumsum())
    fr = np.asarray(freqs, dtype=np.float64)
    # VisCoupling: an (N, N) matrix of lengths, either sign
    vecs = 30 * rng.normal(size=(5, 3))
    length = np.linalg.norm(vecs[None, :, :] - vecs[:, None, :], axis=-1)
    got = cal._coupling_delay(length, freqs, min_dly, sign, c)
    if min_dly is not None:
        length = np.maximum(length, min_dly)
    phase = 2 * np.pi * sign * (fr - fr[0])[None, None, :] / c * length[:, :, None]
    assert got.dtype == np.complex128 and got.shape == (5, 5, Nf) and np.array_equal(got, np.exp(1j * phase))
    # RedVisCoupling: a list of lengths, the sign written as none at all
    length = np.linalg.norm(vecs, axis=-1)
    got = cal._coupling_delay(length, freqs, min_dly, sign, c)
    if min_dly is not None:
        length = np.maximum(length, min_dly)
    phase = 2 * np.pi * (fr - fr[0])[None, :] / c * length[:, None]
    want = np.exp(1j * phase) if sign == 1 else np.exp(-1j * phase)
    assert got.shape == (5, Nf) and np.array_equal(got, want)
    if min_dly is not None:
        assert (length >= min_dly).all() and (np.linalg.norm(vecs, axis=-1) < min_dly).any()


@pytest.mark.parametrize('min_dly', [None, 20.0])
def test_setup_coupling_sets_the_same_delay_phasor_as_before(min_dly):
    """`dly` of the two classes against the expressions their setup_coupling()s held, bit for bit in float64"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        antpos, _, _, _, _, freqs = ct.hex7()
        fr = np.asarray(freqs, dtype=np.float64)
        vecs = np.stack([np.asarray(antpos[a], dtype=np.float64) for a in antpos.keys()])
        clamp = (lambda x: x) if min_dly is None else (lambda x: np.maximum(x, min_dly))
        for conj in (True, False):
            m, _ = ct.build('VisCoupling', setup=False)
            m.setup_coupling(min_dly=min_dly, conj=conj)
            length = clamp(np.linalg.norm(vecs[None, :, :] - vecs[:, None, :], axis=-1))
            phase = 2 * np.pi * (1 if conj else -1) * (fr - fr[0])[None, None, :] / m.c * length[:, :, None]
            assert m.dly.dtype == torch.complex128 and m.dly.shape == (1, 1, 7, 7, 1, ct.NF)
            assert np.array_equal(m.dly.numpy(), np.exp(1j * phase)[None, None, :, :, None, :])
        m, _ = ct.build('RedVisCoupling', setup=False)
        m.setup_coupling(min_dly=min_dly)
        where = {a: i for i, a in enumerate(antpos.keys())}
        length = clamp(np.array([np.linalg.norm(vecs[where[a2]] - vecs[where[a1]]) for a1, a2 in m.coupling_terms]))
        phase = 2 * np.pi * (fr - fr[0])[None, :] / m.c * length[:, None]
        assert np.array_equal(m.dly.numpy(), np.exp(1j * phase)[None, None, :, None, :])
    finally:
        torch.set_default_dtype(old)


def test_check_bls_raises_the_three_errors_in_their_order():
    known = {0, 1, 2}
    cal._check_bls([(0, 0), (0, 1), (1, 2)], known, 'X')
    with pytest.raises(ValueError, match=r'baseline \(0, 3\) names an antenna that is not in antpos'):
        cal._check_bls([(0, 1), (0, 3)], known, 'X')
    with pytest.raises(ValueError, match=r'baseline \(2, 1\): SomeClass needs ant2 >= ant1'):
        cal._check_bls([(0, 1), (2, 1)], known, 'SomeClass')
    with pytest.raises(ValueError, match=r'baseline \(0, 1\) appears twice'):
        cal._check_bls([(0, 1), (1, 2), [0, 1]], known, 'X')
    # reversed and listed twice: its first appearance is already refused as reversed
    with pytest.raises(ValueError, match='needs ant2 >= ant1'):
        cal._check_bls([(2, 1), (2, 1)], known, 'X')
    # reversed with an unknown antenna: the unknown antenna is named
    with pytest.raises(ValueError, match='not in antpos'):
        cal._check_bls([(5, 1)], known, 'X')
    # and the two classes say the same through setup_coupling()
    for name in ('VisCoupling', 'RedVisCoupling'):
        m, _ = ct.build(name, setup=False)
        if name == 'VisCoupling':
            m.bls = [(2, 1), (2, 1)]
        else:
            m.bls_out = [(2, 1), (2, 1)]
        with pytest.raises(ValueError, match=r'baseline \(2, 1\): %s needs ant2 >= ant1' % name):
            m.setup_coupling()


def same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, (int, float, str, bool, type(None), torch.device, torch.dtype)):
        return a == b
    if hasattr(a, '__dict__'):                                 # responses, plans, AntposDict: by their attributes
        return type(a) is type(b) and same(vars(a), vars(b))
    return type(a) is type(b)


@pytest.mark.parametrize('name', ct.CLASSES)
def test_pickle_leaves_the_cached_output_behind(name):
    m, _ = ct.build(name, p0=True)
    m._vd = 'cached output'
    other = pickle.loads(pickle.dumps(m))
    assert other._vd is None and m._vd == 'cached output'
    a, b = dict(vars(m)), dict(vars(other))
    a.pop('_vd'), b.pop('_vd')
    assert list(a) == list(b)
    for k in a:
        assert same(a[k], b[k]), k
    assert isinstance(other.params, torch.nn.Parameter) and torch.equal(other.params.detach(), m.params.detach())
