"""
CPU-side checks of the partly redundant inflation (calibration.PartialRedVisInflate, ops.PartRedPlan, rime_partred_fwd /
_bwd_data / _bwd_coeff, dataset.RedVisAvg): the plan tables against a brute-force listing, the float64 restatement of
tests/partred_common.py against the reference's recorded results (tests/golden/partred.npz) within the derived bound, every
rejected input, the reject codes of the three entry points without a launch, the refusal of CPU tensors, and the kernel names
and the no-scratch property of the built kernels.
"""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

import kernel_asm
import partred_common as pc


def all_cases():
    for name, c in pc.GOLDEN_CASES.items():
        yield name, c['lists'], None
    for name, c in pc.KERNEL_CASES.items():
        yield name, pc.case_lists(c), c['Nin']


@pytest.mark.parametrize('name', list(pc.GOLDEN_CASES) + list(pc.KERNEL_CASES))
def test_plan_tables_against_a_brute_force_listing(name):
    from bayeslim_amd import ops
    lists, Nin = {n: (l, k) for n, l, k in all_cases()}[name]
    rows, cols, _ = pc.entry_list(lists)
    Nout, Nin = len(lists), (int(cols.max()) + 1 if Nin is None else Nin)
    plan = ops.PartRedPlan(rows, cols, Nout, Nin)
    P = pc.build_plan(rows, cols, Nout, Nin)
    for k in ops.PartRedPlan._TABLES:
        assert getattr(plan, k).dtype == np.int32 and getattr(plan, k).tolist() == P[k].tolist(), k
    assert (plan.Nout, plan.Nin, plan.Nnz, plan.max_row, plan.max_col) == (Nout, Nin, len(rows), P['Lrow'], P['Lcol'])
    # every entry exactly once in the row list and once in the column list, members ascending
    assert plan.roff[0] == 0 and plan.roff[-1] == plan.Nnz and plan.coff[0] == 0 and plan.coff[-1] == plan.Nnz
    assert sorted(plan.cmem.tolist()) == list(range(plan.Nnz))
    for i in range(Nout):
        assert all(plan.row[e] == i for e in range(plan.roff[i], plan.roff[i + 1]))
    for j in range(Nin):
        m = plan.cmem[plan.coff[j]:plan.coff[j + 1]].tolist()
        assert m == sorted(m) and all(plan.col[e] == j for e in m)
    T = plan.tables('cpu')
    assert plan.tables('cpu') is T and all(t.dtype == torch.int32 and t.is_contiguous() for t in T.values())
    Q = pickle.loads(pickle.dumps(plan))
    assert '_tabs' not in Q.__dict__ and Q.cmem.tolist() == plan.cmem.tolist()


def test_plan_rejects_bad_tables():
    from bayeslim_amd import ops
    for rows, cols, Nout, Nin in (([0, 1], [0, -1], 2, 2), ([0, 1], [0, 2], 2, 2), ([0, 2], [0, 1], 2, 2), ([0, -1], [0, 1], 2, 2),
                                  ([0, 0], [1, 1], 2, 2), ([], [], 2, 2), ([1, 0], [0, 1], 2, 2), ([0, 1], [0], 2, 2),
                                  ([0.5], [0], 2, 2), ([0], [0], 0, 2), ([0], [0], 2, 0)):
        with pytest.raises(ValueError):
            ops.PartRedPlan(rows, cols, Nout, Nin)


@pytest.mark.parametrize('name', list(pc.GOLDEN_CASES))
def test_restatement_against_the_reference_fixture(name):
    """the float64 restatement on the recorded inputs against the reference's output and gradients of sum w |out|^2: both
    sides float64; the cotangent comes from the output, so its roundings are added (module docstring of partred_common)"""
    g, case = pc.golden(), pc.GOLDEN_CASES[name]
    rows, cols, Nred = pc.entry_list(case['lists'])
    assert (g['idx_' + name] == np.stack([rows, cols])).all() and (g['Nred_' + name] == Nred).all()
    Nout, Nin = (int(x) for x in g['Ashape_' + name])
    assert (Nout, Nin) == (len(case['lists']), int(cols.max()) + 1) and str(g['R_' + name]) == (case['R'] or 'identity')
    R, dR = pc.RESPONSES[case['R']]
    x = g['params_' + name] + (g['p0_' + name] if case['p0'] else 0.0)
    if not case['params']:
        assert (g['params_' + name] == 1.0 / Nred).all()
    c, V, w = R(x), g['data_' + name], g['w_' + name]
    out, _, _ = pc.evaluate(c, V, rows, cols, Nout)
    _, gV, gc = pc.evaluate(c, V, rows, cols, Nout, G=2 * w * out)
    P = pc.build_plan(rows, cols, Nout, Nin)
    L = V.shape[0] * V.shape[1] * V.shape[3] * V.shape[4]
    n = pc.roundings(P, L, Nout, Nin)
    Mo, _, _ = pc.magnitudes(c, V, rows, cols, Nout)
    _, Mv, Mc = pc.magnitudes(c, V, rows, cols, Nout, G=2 * w * Mo)
    fwd = n['numpy'][0] + n['fixture'][0] + 2
    worst = dict(out=pc.ratio(out, g['V_' + name], pc.bound(Mo, n['numpy'][0], 'f64', n['fixture'][0])),
                 gd=pc.ratio(gV, g['gd_' + name], pc.bound(Mv, n['numpy'][1], 'f64', n['fixture'][1], extra=fwd)),
                 gp=pc.ratio(gc * dR(x), g['gp_' + name],
                             pc.bound(Mc * np.abs(dR(x)), n['numpy'][2], 'f64', n['fixture'][2], extra=fwd + pc.CHAIN)))
    print(name, 'worst error / bound:', worst)
    assert max(worst.values()) <= 1.0, worst
    assert int(g['csr_ran']) == 1


def _module(name, **kw):
    from bayeslim_amd import calibration as cal
    case = pc.GOLDEN_CASES[name]
    return cal.PartialRedVisInflate(dict(zip(case['new_bls'], case['lists'])), list(case['new_bls']), **kw)


def test_module_attributes_and_entry_order():
    from bayeslim_amd import calibration as cal
    for name, case in pc.GOLDEN_CASES.items():
        rows, cols, Nred = pc.entry_list(case['lists'])
        m = _module(name)
        assert m.idx.tolist() == [rows.tolist(), cols.tolist()] and m.Nred.tolist() == Nred.tolist()
        assert m.Ashape == (len(case['lists']), int(cols.max()) + 1) and m.new_bls == list(case['new_bls'])
        assert isinstance(m.params, torch.nn.Parameter) and torch.equal(m.params.detach(), torch.ones(len(rows)) / torch.as_tensor(Nred))
        assert m.p0 is None and m.device is None and m.use_csr is True and m.R(3) == 3
        assert m.plan.col.tolist() == cols.tolist() and m.plan.roff.tolist() == pc.build_plan(rows, cols, *m.Ashape)['roff'].tolist()
    # numpy integers count as a list of one, like Python integers
    a = cal.PartialRedVisInflate({(0, 1): np.int64(2), (0, 2): 1, (1, 2): [0, np.int32(2)]}, [(0, 1), (0, 2), (1, 2)], parameter=False)
    assert a.idx.tolist() == [[0, 1, 2, 2], [2, 1, 0, 2]] and a.Nred.tolist() == [1, 1, 2, 2] and not isinstance(a.params, torch.nn.Parameter)
    # a baseline with an empty list is a row without entries
    e = cal.PartialRedVisInflate({(0, 1): [1], (0, 2): []}, [(0, 1), (0, 2)])
    assert e.Ashape == (2, 2) and e.plan.roff.tolist() == [0, 1, 1]


def test_use_csr_changes_nothing():
    a, b = _module('p2_unsorted', use_csr=True), _module('p2_unsorted', use_csr=False)
    assert (a.use_csr, b.use_csr) == (True, False)
    assert torch.equal(a.idx, b.idx) and torch.equal(a.params, b.params) and a.Ashape == b.Ashape
    for k in a.plan._TABLES:
        assert getattr(a.plan, k).tolist() == getattr(b.plan, k).tolist()
    assert type(a).forward is type(b).forward


def test_module_rejects_bad_input():
    from bayeslim_amd import calibration as cal, dataset
    bls = [(0, 1), (0, 2)]
    with pytest.raises(KeyError):
        cal.PartialRedVisInflate({(0, 1): [0]}, bls)
    with pytest.raises(ValueError, match='negative'):
        cal.PartialRedVisInflate({(0, 1): [0], (0, 2): [1, -1]}, bls)
    with pytest.raises(ValueError, match='twice'):
        cal.PartialRedVisInflate({(0, 1): [0], (0, 2): [1, 0, 1]}, bls)
    with pytest.raises(ValueError, match='no entry'):
        cal.PartialRedVisInflate({(0, 1): [], (0, 2): []}, bls)
    with pytest.raises(ValueError, match='entries'):
        cal.PartialRedVisInflate({(0, 1): [0], (0, 2): [1, 0]}, bls, params=torch.ones(4))
    m = cal.PartialRedVisInflate({(0, 1): [0], (0, 2): [1, 0]}, bls)
    vd = dataset.VisData()
    vd.setup_meta(None, None)
    vd.setup_data([(0, 0), (1, 1), (2, 2)], torch.arange(2.0), torch.linspace(1e8, 2e8, 4), pol='ee',
                  data=torch.zeros(1, 1, 3, 2, 4, dtype=torch.complex64))
    with pytest.raises(ValueError, match='baselines'):
        m(vd)


def test_cpu_tensors_are_refused():
    from bayeslim_amd import calibration as cal, dataset, ops
    plan = ops.PartRedPlan([0, 1, 1], [0, 1, 0], 2, 2)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ops.partred_inflate(torch.zeros(1, 1, 2, 2, 4, dtype=torch.complex64), torch.ones(3), plan)
    m = cal.PartialRedVisInflate({(0, 1): [0], (0, 2): [1, 0]}, [(0, 1), (0, 2)])
    vd = dataset.VisData()
    vd.setup_meta(None, None)
    vd.setup_data([(0, 0), (1, 1)], torch.arange(2.0), torch.linspace(1e8, 2e8, 4), pol='ee',
                  data=torch.zeros(1, 1, 2, 2, 4, dtype=torch.complex64))
    with pytest.raises(RuntimeError, match='needs tensors on the GPU'):
        m(vd)


def test_push_pickle_and_deepcopy_on_the_host():
    m = _module('p1_exp', p0=torch.full((11,), 0.25), R=torch.exp)
    m.plan.tables('cpu')
    for q in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert '_tabs' not in q.plan.__dict__ and q._vd is None and torch.equal(q.params, m.params) and torch.equal(q.idx, m.idx)
        assert q.R is torch.exp and torch.equal(q.p0, m.p0)
    assert pickle.loads(pickle.dumps(_module('p1_sorted'))).R(2.5) == 2.5              # the default response pickles
    m.push(torch.float64)
    assert m.params.dtype == torch.float64 and m.p0.dtype == torch.float64 and isinstance(m.params, torch.nn.Parameter)
    assert m.idx.dtype == torch.int64 and m.device is None
    m.push('cpu')
    assert m.device == 'cpu' and 'cpu' in m.plan._cache()


def test_entry_points_reject_bad_arguments_without_launching():
    """the acceptable call is never made: the pointers are those of a small host buffer"""
    from bayeslim_amd._lib import lib
    buf = ctypes.create_string_buffer(4096)
    one = ctypes.c_void_p(ctypes.addressof(buf))

    def fwd(dtype=0, NP=1, V=one, c=one, roff=one, col=one, Nout=2, Nin=2, Nnz=3, Nt=3, Nf=5, st=(30, 15, 5, 1), out=one):
        return lib.rime_partred_fwd(dtype, NP, V, c, roff, col, Nout, Nin, Nnz, Nt, Nf, *st, out, None)

    def bwd_data(dtype=0, NP=1, G=one, c=one, row=one, coff=one, cmem=one, Nout=2, Nin=2, Nnz=3, Nt=3, Nf=5, gV=one):
        return lib.rime_partred_bwd_data(dtype, NP, G, c, row, coff, cmem, Nout, Nin, Nnz, Nt, Nf, gV, None)

    def bwd_coeff(dtype=0, NP=1, V=one, G=one, roff=one, col=one, Nout=2, Nin=2, Nnz=3, Nt=3, Nf=5, st=(30, 15, 5, 1), gc=one):
        return lib.rime_partred_bwd_coeff(dtype, NP, V, G, roff, col, Nout, Nin, Nnz, Nt, Nf, *st, gc, None)

    ptrs = {fwd: ('V', 'c', 'roff', 'col', 'out'), bwd_data: ('G', 'c', 'row', 'coff', 'cmem', 'gV'),
            bwd_coeff: ('V', 'G', 'roff', 'col', 'gc')}
    for fn, names in ptrs.items():
        for dtype in (2, 7, -1):
            assert fn(dtype=dtype) == -1, (fn.__name__, dtype)
        for k in names:
            assert fn(**{k: None}) == -1, (fn.__name__, k)
        for k in ('Nout', 'Nin', 'Nnz', 'Nt', 'Nf'):
            assert fn(**{k: 0}) == -1 and fn(**{k: -2}) == -1, (fn.__name__, k)
        for NP in (0, 3, -1):
            assert fn(NP=NP) == -1, (fn.__name__, NP)
        assert fn(dtype=7, **{names[0]: None}) == -1
    for fn in (fwd, bwd_coeff):
        for k in range(4):
            st = [30, 15, 5, 1]
            st[k] = -1
            assert fn(st=tuple(st)) == -1, (fn.__name__, k)


def test_partred_kernels_are_the_only_ones_and_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/partred.hip: 4 forward (precision x Npol), 2 gradient-of-data and 2
    gradient-of-coefficient kernels, every one a partred_ kernel, no private segment in any"""
    asm, kernels, sizes = kernel_asm.read('partred')
    assert len(kernels) == 8 and all('partred_' in k for k in kernels), kernels
    assert len(sizes) == 8 and max(sizes) == 0, sizes


def test_redvisavg_is_bl_average():
    from bayeslim_amd import dataset, utils
    rng = np.random.default_rng(3651)
    bls = [(0, 1), (1, 2), (0, 2), (2, 3), (1, 3)]
    reds = [[(0, 1), (1, 2), (2, 3)], [(0, 2), (1, 3)]]
    vd = dataset.VisData()
    vd.setup_meta(None, utils.AntposDict(pc.ANTS, pc.ANTVECS))
    data = torch.as_tensor(rng.normal(size=(1, 1, 5, 3, 4)) + 1j * rng.normal(size=(1, 1, 5, 3, 4)))
    vd.setup_data(bls, torch.arange(3.0), torch.linspace(1e8, 2e8, 4), pol='ee', data=data)
    w = torch.as_tensor(rng.uniform(0.5, 2.0, size=(1, 1, 5, 3, 4)))
    for wgts in (None, w):
        blk = dataset.RedVisAvg(reds, wgts=wgts)
        assert (blk.reds, blk.inplace, blk.device) == (reds, False, None)
        a, b, c = blk(vd), vd.bl_average(reds=reds, wgts=wgts), blk.forward(vd, prior_cache={})
        assert a is not vd and a.bls == [(0, 1), (0, 2)] and torch.equal(a.data, b.data) and torch.equal(c.data, b.data)
        assert tuple(a.data.shape) == (1, 1, 2, 3, 4)
    assert torch.allclose(a.data[0, 0, 1], (w[0, 0, 2] * data[0, 0, 2] + w[0, 0, 4] * data[0, 0, 4]) / (w[0, 0, 2] + w[0, 0, 4]))
    blk = dataset.RedVisAvg(reds, wgts=w, device='cpu')
    blk.push(torch.float32)
    assert blk.wgts.dtype == torch.float32 and blk.device == 'cpu'
    blk.push('cpu')
    assert blk.device == 'cpu'
    blk = dataset.RedVisAvg(reds, inplace=True)
    v2 = vd.copy(copydata=True)
    assert blk(v2) is v2 and v2.data.shape[2] == 2
