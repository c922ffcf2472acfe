"""
The host call layer the plan-driven ops share (ops._IndexPlan, _timed, _workspace, _dtype_code, _host_array): what the device
tables of a plan hold and how they travel, what the profile recorder appends, and what the small converters accept.  No GPU.
"""
import copy
import pickle

import numpy as np
import pytest
import torch

from bayeslim_amd import ops

C = ops.COUPLING_CONJ
PLANS = {
    # every table of every plan non-trivial at the smallest size: two groups and the identity over two times; an empty bin;
    # a row read plain at (0, 1) and conjugated at (1, 0); term 0 with three words, i.e. two segments of two
    'redvis': (lambda: ops.RedVisPlan(red=[1, 0, 1], Nred=2, Ntm=2), ('red', 'tmap', 'goff', 'gmem', 'toff', 'tmem')),
    'timeavg': (lambda: ops.TimeAvgPlan([[0, 2], [], [1]], Nt=3), ('bin_ptr', 'members', 't_ptr', 't_pos', 'pos_bin')),
    'coupling': (lambda: ops.CouplingPlan([[0, 1], [1 | C, -1]], [0, 1, 2], Nbl=2), ('table', 'otab', 'ftab')),
    'redcoupling': (lambda: ops.RedCouplingPlan(row=[0, 1, 1], col=[0, 1, 0], conj=[0, 1, 0], a=[0, 0, 1], b=[0, -1, -1],
                                                Nout=2, Nin=2, Nterms=2, seg=2),
                    ('ent', 'roff', 'coff', 'cmem', 'toff', 'tmem', 'segterm', 'segstart', 'tsoff')),
}


def same_arrays(p, q):
    keys = [k for k, v in p.__dict__.items() if isinstance(v, np.ndarray)]
    return len(keys) > 0 and all(np.array_equal(getattr(p, k), getattr(q, k)) and getattr(p, k).dtype == getattr(q, k).dtype
                                 for k in keys)


@pytest.mark.parametrize('name', sorted(PLANS))
def test_tables_and_pickling(name):
    make, names = PLANS[name]
    plan = make()
    assert tuple(plan._TABLES) == names
    if name == 'redcoupling':
        assert plan.tsoff.tolist() == [0, 2, 3] and plan.Nseg == 3
    T = plan.tables('cpu')
    assert isinstance(T, dict) and set(T) == set(names)
    for k in names:
        host = getattr(plan, k)
        assert T[k].dtype == torch.int32 and T[k].is_contiguous() and T[k].device.type == 'cpu'
        assert tuple(T[k].shape) == host.shape and np.array_equal(T[k].numpy(), host)
    assert plan.tables('cpu') is T and plan.tables(torch.device('cpu')) is T
    other = plan.tables('cpu:0')                               # another device string: an entry of its own
    assert other is not T and set(plan.__dict__['_tabs']) == {'cpu', 'cpu:0'}
    again = pickle.loads(pickle.dumps(plan))
    assert '_tabs' in plan.__dict__ and '_tabs' not in again.__dict__ and same_arrays(plan, again)
    assert same_arrays(plan, copy.deepcopy(plan))
    assert set(again.tables('cpu')) == set(names)


class FakeEvent:
    log = []

    def __init__(self, enable_timing=False):
        assert enable_timing
        self.records = 0
        FakeEvent.log.append(('new', self))

    def record(self):
        self.records += 1
        FakeEvent.log.append(('record', self))


@pytest.fixture
def fake_events(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'Event', FakeEvent)
    monkeypatch.setattr(FakeEvent, 'log', [])
    return FakeEvent.log


def test_recorder_off(fake_events, monkeypatch):
    monkeypatch.setattr(ops, 'PROFILE', None)
    with ops._timed('k', 1, 2) as late:
        fake_events.append('body')
    assert fake_events == ['body'] and late is None            # no event, and the body is told so


def test_recorder_appends_one_tuple(fake_events, monkeypatch):
    prof = []
    monkeypatch.setattr(ops, 'PROFILE', prof)
    with ops._timed('k', 7, 'x'):
        fake_events.append('body')
        monkeypatch.setattr(ops, 'PROFILE', None)              # read once, on entry
        assert prof == []
    assert len(prof) == 1 and len(prof[0]) == 5
    name, e0, e1, a, b = prof[0]
    assert (name, a, b) == ('k', 7, 'x') and e0 is not e1 and (e0.records, e1.records) == (1, 1)
    assert [x for x in fake_events if x == 'body' or x[0] == 'record'] == [('record', e0), 'body', ('record', e1)]


def test_recorder_fields_of_the_body(fake_events, monkeypatch):
    """the fringe tuples carry the flop count, which only the launches know: the body appends to the list it is given"""
    prof = []
    monkeypatch.setattr(ops, 'PROFILE', prof)
    with ops._timed('fringe_ant_fwd_kernel', 10) as late:
        assert late == []
        late += (20, 30)
    assert prof[0][0] == 'fringe_ant_fwd_kernel' and prof[0][3:] == (10, 20, 30) and len(prof[0]) == 6


def test_recorder_body_raises(fake_events, monkeypatch):
    prof = []
    monkeypatch.setattr(ops, 'PROFILE', prof)
    with pytest.raises(KeyError, match='boom'):
        with ops._timed('k', 1):
            raise KeyError('boom')
    assert prof == [] and sum(x[0] == 'record' for x in fake_events) == 1


def test_dtype_code():
    for dt in (torch.float32, torch.complex64):
        assert ops._dtype_code(dt) == ops.RIME_F32 and ops._real_dtype(torch.empty(0, dtype=dt)) == (ops.RIME_F32, torch.float32)
    for dt in (torch.float64, torch.complex128):
        assert ops._dtype_code(dt) == ops.RIME_F64 and ops._real_dtype(torch.empty(0, dtype=dt)) == (ops.RIME_F64, torch.float64)
    assert ops.RIME_F32 != ops.RIME_F64
    for dt in (torch.float16, torch.bfloat16, torch.int32, torch.bool):
        with pytest.raises(TypeError, match='unsupported dtype %s' % dt):
            ops._dtype_code(dt)
        with pytest.raises(TypeError, match='unsupported dtype %s' % dt):
            ops._real_dtype(torch.empty(0, dtype=dt))


def test_host_array():
    want = np.array([[3, 1], [2, 0]])
    for x in (want.tolist(), want, want.astype(np.int32), torch.as_tensor(want), torch.as_tensor(want).to(torch.int16)):
        a = ops._host_array(x)
        assert isinstance(a, np.ndarray) and a.shape == (2, 2) and np.array_equal(a, want)
        assert np.issubdtype(a.dtype, np.integer)
        f = ops._host_array(x, flat=True, integer='indices must be integers')
        assert f.shape == (4,) and f.tolist() == [3, 1, 2, 0]
    mask = ops._host_array(np.array([True, False, True]))
    assert mask.dtype == bool and mask.tolist() == [True, False, True]          # filt_tables and RedCouplingPlan tell it apart
    assert ops._host_array(torch.tensor([True, False])).dtype == bool
    assert ops._host_array([0.5, 1.0]).dtype == np.float64                       # no check asked for: as numpy reads it
    assert ops._host_array([], flat=True, integer='never').size == 0             # an empty bin is no error
    for bad in ([0.5], np.array([1.0, 2.0]), torch.tensor([1.0]), np.array([True])):
        with pytest.raises(ValueError, match='indices must be integers'):
            ops._host_array(bad, integer='indices must be integers')
