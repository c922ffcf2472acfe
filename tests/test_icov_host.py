"""
Axis covariances without a GPU: optim.apply_icov / cov_get_diag / compute_icov and TensorData.compute_icov on the CPU against
the float64 oracle of icov_common.py, the (O, n, I) mapping against an independent recomputation, the launch planner of
csrc/icov.hip (rime_icov_plan) and the return codes of the rejected calls of its entry points.
"""
import ctypes

import numpy as np
import pytest
import torch

import icov_common as ic
from bayeslim_amd import _lib, dataset, ops, optim

C128 = torch.complex128
CASES = list(range(len(ic.CASES)))


def test_oracle_einsum_equals_the_loop_over_batches():
    """the oracle's einsums (the issue's table) against r.conj() @ W[b] @ r, batch by batch"""
    for c in CASES:
        pred, data, icov = ic.public_problem(c, C128)
        a, b = ic.oracle_einsum(c, pred - data, icov), ic.oracle_loop(c, pred - data, icov)
        assert a.shape == b.shape == ic.CASES[c][4]
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


@pytest.mark.parametrize('case', CASES, ids=ic.CASE_IDS)
def test_apply_icov_on_the_cpu_against_the_loop_oracle(case):
    mode, cov_axis, shape, icov_shape, out_shape, _ = ic.CASES[case]
    pred, data, icov = ic.public_problem(case, C128)
    assert icov.shape == icov_shape                       # 'time': (Npol, Npol, Nbl, Nf, Nt, Nt), the documented shape
    res = pred - data
    out = optim.apply_icov(res, icov, cov_axis, mode=mode)
    ref = ic.oracle_loop(case, res, icov)
    assert out.shape == out_shape and out.is_complex()    # what einsum returns
    assert float((out.real - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float(out.imag.abs().max()) <= 1e-12 * float(ref.abs().max())
    chisq, r = optim.forward_chisq(pred, data, icov, cov_axis, mode=mode)          # CPU: the torch path, real, with residual
    assert not chisq.is_complex() and torch.equal(r, res)
    assert abs(float(chisq) - float(ref.sum())) <= 1e-12 * float(ref.sum())
    per, _ = optim.forward_chisq(pred, data, icov, cov_axis, sum_chisq=False, mode=mode)
    assert per.shape == out_shape and not per.is_complex()


def test_apply_icov_time_takes_the_documented_shape_not_the_reference_equation():
    """Nt != Nf: an icov in the layout the reference's equation indexes (ijkln: Nbl, Nt, Nt) is not accepted"""
    case = ic.CASE_IDS.index('vis-time')
    pred, data, icov = ic.public_problem(case, C128)
    with pytest.raises(RuntimeError):
        optim.apply_icov(pred, icov[..., 0, :, :].expand(2, 2, 5, 4, 4), 'time')
    assert optim.apply_icov(pred, icov, 'time').shape == (2, 2, 5, 6)


def test_apply_icov_unknown_axis_and_unchanged_branches():
    x = torch.randn(2, 2, 3, 2, 2, dtype=C128)
    with pytest.raises(NameError):
        optim.apply_icov(x, x, 'lst')
    with pytest.raises(NameError):
        optim.apply_icov(x, x, 'pix')                     # a map axis with mode 'vis'
    with pytest.raises(NameError):
        optim.cov_get_diag(x, 'lst')
    w = torch.rand(x.shape, dtype=torch.float64)
    assert torch.equal(optim.apply_icov(x, w), x.conj() * x * w) and torch.equal(optim.apply_icov(x, None), x.conj() * x)
    M = torch.randn(x.numel(), x.numel(), dtype=C128)
    assert torch.equal(optim.apply_icov(x, M, 'full'), x.ravel().conj() @ M @ x.ravel())


@pytest.mark.parametrize('case', CASES, ids=ic.CASE_IDS)
def test_cov_get_diag_returns_the_diagonal_in_the_shape_of_the_data(case):
    mode, cov_axis, shape, icov_shape, _, _ = ic.CASES[case]
    diag = torch.arange(1.0, 1 + int(np.prod(shape)), dtype=torch.float64).reshape(shape)
    cov = torch.diag_embed(diag.moveaxis(ic.AXIS[(mode, cov_axis)], -1))
    assert cov.shape == icov_shape
    assert torch.equal(optim.cov_get_diag(cov, cov_axis, mode=mode), diag)
    assert optim.cov_get_diag(diag, None) is diag
    N = diag.numel()
    assert torch.equal(optim.cov_get_diag(torch.diag(diag.ravel()), 'full', shape=shape), diag)
    assert N == int(np.prod(shape))


@pytest.mark.parametrize('inv', ['pinv', 'inv', 'chol'])
def test_compute_icov_inverts_every_matrix(inv):
    for c in CASES:
        mode, cov_axis, _, icov_shape, _, _ = ic.CASES[c]
        cov = ic.public_problem(c, C128)[2]
        icov = optim.compute_icov(cov, cov_axis, inv=inv)
        eye = torch.eye(icov_shape[-1], dtype=C128).expand(icov_shape)
        assert icov.shape == icov_shape and float((icov @ cov - eye).abs().max()) < 1e-10
    full = ic.public_problem(0, C128)[2][0, 0, 0, 0]
    assert float((optim.compute_icov(full, 'full', inv=inv) @ full - torch.eye(5, dtype=C128)).abs().max()) < 1e-10
    var = torch.tensor([0.0, 0.5, 4.0], dtype=torch.float64)
    assert torch.equal(optim.compute_icov(var, None, inv=inv), 1 / var.clip(1e-40))
    with pytest.raises(ValueError):
        optim.compute_icov(full, 'full', inv='lu')
    with pytest.raises(NameError):
        optim.compute_icov(ic.public_problem(0, C128)[2], 'lst')


def test_tensordata_compute_icov_sets_icov():
    for c in (ic.CASE_IDS.index('vis-freq'), ic.CASE_IDS.index('map-pix')):
        mode, cov_axis, shape, icov_shape, _, _ = ic.CASES[c]
        pred, data, cov = ic.public_problem(c, C128)
        td = dataset.VisData() if mode == 'vis' else dataset.MapData()
        td.data = data
        td.set_cov(cov, cov_axis)
        assert td.icov is None and td.cov_ndim == data.numel()
        td.compute_icov()
        eye = torch.eye(icov_shape[-1], dtype=C128).expand(icov_shape)
        assert td.icov.shape == icov_shape and float((td.icov @ cov - eye).abs().max()) < 1e-10
        td.compute_icov(inv='chol')
        assert float((td.icov @ cov - eye).abs().max()) < 1e-10
    td = dataset.TensorData()
    td.data = torch.ones(3, dtype=torch.float64)
    td.set_cov(torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64), None)
    td.compute_icov()
    assert torch.equal(td.icov, torch.tensor([1.0, 0.5, 0.25], dtype=torch.float64))


@pytest.mark.parametrize('case', CASES, ids=ic.CASE_IDS)
def test_layout_mapping_against_moveaxis_and_reshape(case):
    """ops.cov_axis_layout: the data as (O, n, I) and icov as (O I, n, n), batch o I + i, reproduce the oracle"""
    mode, cov_axis, shape, icov_shape, out_shape, _ = ic.CASES[case]
    axis, O, n, I, ishape, oshape = ops.cov_axis_layout(shape, cov_axis, mode)
    assert (axis, ishape, oshape) == (ic.AXIS[(mode, cov_axis)], icov_shape, out_shape)
    assert O == int(np.prod(shape[:axis])) and n == shape[axis] and I == int(np.prod(shape[axis + 1:])) and O * n * I == np.prod(shape)
    pred, data, icov = ic.public_problem(case, C128)
    res = pred - data
    r3 = res.reshape(O, n, I)                                        # the kernel's view: a reshape of the dense data
    W = icov.reshape(O * I, n, n)
    q = torch.zeros(O * I, dtype=torch.float64)
    for o in range(O):
        for i in range(I):
            q[o * I + i] = (r3[o, :, i].conj() @ W[o * I + i] @ r3[o, :, i]).real
    ref = ic.oracle_einsum(case, res, icov)
    assert float((q.reshape(out_shape) - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # independently: covariance axis moved last, batch axes flattened in data order
    rb = res.moveaxis(axis, -1).reshape(O * I, n)
    assert torch.equal(rb, r3.permute(0, 2, 1).reshape(O * I, n))
    with pytest.raises(NameError):
        ops.cov_axis_layout(shape, 'lst', mode)
    with pytest.raises(ValueError):
        ops.cov_axis_layout(shape + (2,), cov_axis, mode)


@pytest.mark.parametrize('dtype', [torch.complex64, torch.complex128], ids=['c64', 'c128'])
@pytest.mark.parametrize('n', ic.PLAN_N)
def test_planner(n, dtype):
    cb = 8 if dtype == torch.complex64 else 16
    for O, I in ((1, 1), (5, 1), (2, 1), (1, 3), (5, 9), (20000, 1), (1000, 60), (1, 64), (300000, 1)):
        p = ops.icov_plan(dtype, O, n, I)
        assert p['lanes'] in (8, 16, 32, 64) and 64 % p['lanes'] == 0
        assert p['vec'] == (2 if dtype == torch.complex64 and n % 2 == 0 else 1) and p['vec'] * cb in (8, 16)
        nv = n // p['vec']
        assert p['lanes'] == 64 or (nv <= p['lanes'] and (p['lanes'] == 8 or nv > p['lanes'] // 2))   # the smallest that covers a row
        T = p['tile']
        assert 1 <= T <= 256 and T & (T - 1) == 0
        assert T * n * cb <= p['stage_bytes'] <= p['stage_limit'] == 64 * 1024
        assert p['lds_bytes'] == p['stage_bytes'] + 8 * (p['rows_per_split'] * T + 256) <= 160 * 1024
        assert p['tile_along_outer'] == int(I == 1)
        # the row splits cover every row exactly once
        rows = [a for s in range(p['splits']) for a in range(s * p['rows_per_split'], min(n, (s + 1) * p['rows_per_split']))]
        assert rows == list(range(n)) and p['rows_per_split'] % 4 == 0
        assert all(s * p['rows_per_split'] < n for s in range(p['splits']))
        tiles = (1 if I == 1 else O) * -(-(O if I == 1 else I) // T)
        assert p['grid'] == min(tiles * p['splits'], 4096)
        assert (p['splits'] > 1) == (tiles < 512 and n > 4)          # fewer than two work-groups per CU: split the rows
        assert _lib.lib.rime_icov_workspace(ops._dtype_code(dtype), O, n, I) == 8 * (4096 + (O * I * p['splits'] if p['splits'] > 1 else 0))
    split = ops.icov_plan(dtype, *ic.SPLIT_SHAPE)
    assert split['splits'] > 1 and split['grid'] >= 64


def test_planner_refuses_an_axis_beyond_the_lds_staging():
    assert ops.icov_plan(torch.complex64, 1, 8190, 1)['stage_bytes'] == 65536
    for dtype, n in ((torch.complex64, 8192), (torch.complex128, 4096)):
        with pytest.raises(ValueError, match='LDS staging'):
            ops.icov_plan(dtype, 1, n, 1)
    out = (ctypes.c_int * 10)()
    assert _lib.lib.rime_icov_plan(0, 1, 8192, 1, out) == -4
    assert _lib.lib.rime_icov_workspace(0, 1, 8192, 1) == 0


# ---- rejected calls (the style of test_valu_rejected_calls.py): each returns before anything is launched -----------------
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -4
_BUF = ctypes.create_string_buffer(4096 + 16)
PTR = (ctypes.addressof(_BUF) + 15) & ~15                              # 16-byte aligned host memory, never dereferenced
_PLAN = (ctypes.c_int * 10)()
WS = _lib.lib.rime_icov_workspace(0, 2, 4, 3)

BASE = {
    'rime_icov_plan': dict(dtype=0, O=2, n=4, I=3, plan_host=_PLAN),
    'rime_icov_fwd': dict(dtype=0, pred=PTR, data=None, icov=PTR, O=2, n=4, I=3, y=PTR, q=PTR, out=PTR, workspace=PTR,
                          workspace_bytes=WS, stream=None),
    'rime_icov_bwd': dict(dtype=0, y=PTR, g=PTR, g_per_batch=0, O=2, n=4, I=3, gpred=PTR, stream=None),
}
ROWS = [
    ('rime_icov_plan', dict(dtype=7), EINVAL), ('rime_icov_plan', dict(dtype=-1), EINVAL), ('rime_icov_plan', dict(n=0), EINVAL),
    ('rime_icov_plan', dict(O=0), EINVAL), ('rime_icov_plan', dict(I=-1), EINVAL), ('rime_icov_plan', dict(plan_host=None), EINVAL),
    ('rime_icov_plan', dict(n=8192), EUNSUPPORTED), ('rime_icov_plan', dict(dtype=7, n=8192), EINVAL),
    ('rime_icov_fwd', dict(n=0), EINVAL), ('rime_icov_fwd', dict(O=0), EINVAL), ('rime_icov_fwd', dict(I=0), EINVAL),
    ('rime_icov_fwd', dict(pred=None), EINVAL), ('rime_icov_fwd', dict(icov=None), EINVAL),
    ('rime_icov_fwd', dict(y=None, q=None, out=None), EINVAL), ('rime_icov_fwd', dict(icov=PTR + 8), EINVAL),
    ('rime_icov_fwd', dict(dtype=7), EINVAL), ('rime_icov_fwd', dict(dtype=-1), EINVAL),
    ('rime_icov_fwd', dict(dtype=1, pred=PTR + 8), EINVAL), ('rime_icov_fwd', dict(dtype=1, y=PTR + 8), EINVAL),   # complex128: 16 bytes
    ('rime_icov_fwd', dict(pred=PTR + 4), EINVAL),
    ('rime_icov_fwd', dict(workspace=None), EWORKSPACE), ('rime_icov_fwd', dict(workspace_bytes=WS - 1), EWORKSPACE),
    ('rime_icov_fwd', dict(workspace_bytes=0), EWORKSPACE),
    ('rime_icov_fwd', dict(dtype=7, workspace=None), EINVAL),            # dtype (the plan needs it) ahead of the workspace
    ('rime_icov_fwd', dict(n=0, workspace=None), EINVAL), ('rime_icov_fwd', dict(pred=None, workspace_bytes=0), EINVAL),
    ('rime_icov_fwd', dict(n=8192), EUNSUPPORTED), ('rime_icov_fwd', dict(n=8192, workspace=None), EUNSUPPORTED),
    ('rime_icov_bwd', dict(n=0), EINVAL), ('rime_icov_bwd', dict(O=-1), EINVAL), ('rime_icov_bwd', dict(I=0), EINVAL),
    ('rime_icov_bwd', dict(y=None), EINVAL), ('rime_icov_bwd', dict(g=None), EINVAL), ('rime_icov_bwd', dict(gpred=None), EINVAL),
    ('rime_icov_bwd', dict(g_per_batch=2), EINVAL), ('rime_icov_bwd', dict(dtype=7), EINVAL), ('rime_icov_bwd', dict(dtype=-1), EINVAL),
    ('rime_icov_bwd', dict(dtype=7, y=None), EINVAL),
]


def _id(row):
    entry, bad, code = row
    return entry[len('rime_'):] + '-' + '-'.join('%s=%s' % (k, 'ptr+8' if v == PTR + 8 else 'ptr+4' if v == PTR + 4 else v) for k, v in bad.items())


def test_rejected_call_table_matches_the_signatures():
    assert ops.icov_plan(torch.complex64, 2, 4, 3)['splits'] == 1 and WS == 8 * 4096      # the partial totals alone
    for entry, args in BASE.items():
        assert len(args) == len(_lib.SIGNATURES[entry][1]), entry
    for entry, bad, code in ROWS:
        assert bad and set(bad) <= set(BASE[entry]) and code != OK
    assert len({_id(r) for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize('row', ROWS, ids=_id)
def test_rejected_call_returns_its_code(row):
    entry, bad, code = row
    args = dict(BASE[entry], **bad)
    assert getattr(_lib.lib, entry)(*args.values()) == code


def test_chisq_axis_has_no_cpu_path_and_takes_constants_only():
    pred, data, icov = ic.public_problem(2, torch.complex64)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ops.chisq_axis(pred, data, icov, 'freq')
    with pytest.raises(ValueError, match='icov requires grad'):
        ops.chisq_axis(pred, data, icov.clone().requires_grad_(True), 'freq')
    with pytest.raises(ValueError, match='data requires grad'):
        ops.chisq_axis(pred, data.clone().requires_grad_(True), icov, 'freq')


@pytest.mark.parametrize('cov_axis', ['freq', 'time', 'bl', None])
def test_logprob_never_copies_an_axis_icov(cov_axis, monkeypatch):
    """LogProb.forward_chisq hands an axis inverse covariance on as the target's own storage, whole and in its documented
    shape (Npol = 1 axes kept), through ONE get_icov call; the diagonal case keeps its one default call"""
    from bayeslim_amd import utils
    shape = (1, 1, 3, 4, 5)
    rng = np.random.default_rng(3)
    data = torch.as_tensor(ic.cnormal(rng, shape))

    class Model(utils.Module):
        def __init__(self):
            super().__init__(name='m')
            self.params = torch.nn.Parameter(torch.as_tensor(ic.cnormal(rng, shape)))

        def forward(self, inp=None, prior_cache=None, **kw):
            td = dataset.TensorData()
            td.data = self.params * 1.0
            return td

    target = dataset.VisData()
    target.setup_data([(0, 1), (0, 2), (1, 2)], torch.arange(4.0), torch.linspace(1e8, 2e8, 5), pol='ee', data=data)
    if cov_axis is None:
        target.set_cov(torch.rand(shape, dtype=torch.float64) + 1, None)
    else:
        ishape = ops.cov_axis_layout(shape, cov_axis, 'vis')[4]
        target.set_cov(torch.as_tensor(ic.hermitian_pd(rng, ishape[:-2], ishape[-1])), cov_axis)
    target.compute_icov()
    calls, seen = [], []
    get_icov, apply_icov = target.get_icov, optim.apply_icov
    monkeypatch.setattr(target, 'get_icov', lambda **kw: calls.append(kw) or get_icov(**kw))
    monkeypatch.setattr(optim, 'apply_icov', lambda res, icov, *a, **kw: seen.append(icov) or apply_icov(res, icov, *a, **kw))
    prob = optim.LogProb(Model(), dataset.Dataset([target]))
    chisq, res = prob.forward_chisq()
    assert len(calls) == 1 and len(seen) == 1 and res is not None
    if cov_axis is None:
        assert calls == [{}]
    else:
        assert calls == [dict(squeeze=False, try_view=True)]
        assert seen[0].data_ptr() == target.icov.data_ptr() and seen[0].shape == target.icov.shape
        r = prob.model.params.detach() - data
        ref = torch.einsum(optim._ICOV_EINSUM[('vis', cov_axis)], r.conj(), target.icov, r).real.sum()
        assert abs(float(chisq) - float(ref)) <= 1e-12 * abs(float(ref))
