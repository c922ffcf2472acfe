"""
GPU tests of the grouped filter kernel (csrc/filt.hip through ops.filt_apply) and of the filter modules (bayeslim_amd/filt.py).

Every instantiation {f32, f64} x {real, complex G} x {plain, residual, input_idx} runs forward and backward against the float64
CPU oracle of tests/filt_common.py (itself pinned to the reference by tests/test_filt_host.py) at the smallest shapes that
reach every path: N in {5, 37, 64, 70} and 130 (two 128-row tiles), Npol^2 in {1, 4}, 6 - 9 baselines x Nt in {1, 5}, 30
baselines x 5 times under one filter (150 lines: three 64-line tiles), three interleaved filters plus unassigned baselines,
and a rectangular 37 x 64 G.  The operands of the oracle are the ROUNDED operands of the run, so the bound measures arithmetic:

    |y - y64| <= tol (sum_k |W_ik| |x_k| + base_i |x_i|)

f32: tol = 2e-6 (the f32 MFMA is an fmaf chain: <= 1.5e-7 sum |a b| at K <= 1024, doubled for the complex product, ~6x margin);
f64: tol = 1e-12 (K eps at K = 1024 with 10x margin).  Elements the kernel must not compute (unfiltered lines, columns
outside input_idx) have scale 0 and must therefore equal the input bit for bit.
"""
import copy
import pickle
import zlib

import numpy as np
import pytest
import torch

from filt_common import golden, oracle_filter, cnormal

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RDT = {'f32': torch.float32, 'f64': torch.float64}
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
TOL = {'f32': 2e-6, 'f64': 1e-12}

# name: (M, K, leading shape, Nbl, Nt, baseline -> filter)
SHAPES = {
    'N5': (5, 5, (1, 1), 6, 1, (0,) * 6),
    'N37_pol4_3filt': (37, 37, (2, 2), 7, 5, (2, 0, -1, 1, 0, 2, 1)),
    'N64_3filt': (64, 64, (1, 1), 9, 5, (1, -1, 0, 2, 2, 0, -1, 1, 0)),
    'N70': (70, 70, (1, 1), 8, 1, (0, 1, 0, 1, -1, 1, 0, 0)),
    'N130_150lines': (130, 130, (1, 1), 30, 5, (0,) * 30),
    'rect37x64': (37, 64, (1, 1), 6, 5, (0, 1, 1, 0, 1, 0)),
}


def make_inputs(name, cplx, mode, prec):
    """(G, x, cot, idx) rounded to the precision of the run, as float64 / complex128 CPU tensors"""
    M, K, lead, Nbl, Nt, b2f = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(repr((name, cplx, mode)).encode()))
    idx = None
    if mode == 'input_idx':
        M = K // 2 + 1 if M == K else M                       # in-painting: M of the K samples are replaced
        idx = np.sort(rng.permutation(K)[:M])
    Nf = max(b2f) + 1
    G = cnormal(rng, Nf, M, K) if cplx else torch.as_tensor(rng.normal(size=(Nf, M, K)))
    G = G / np.sqrt(K)
    x = cnormal(rng, *lead, Nbl, Nt, K)
    Ny = K if idx is not None else M
    cot = cnormal(rng, *lead, Nbl, Nt, Ny)
    rnd = lambda t: t.to(CDT[prec] if t.is_complex() else RDT[prec]).to(torch.complex128 if t.is_complex() else torch.float64)
    return rnd(G), rnd(x), rnd(cot), idx


def run_gpu(G, x, cot, residual, idx, layout, prec):
    from bayeslim_amd import ops
    plan = ops.FiltPlan(G, residual=residual, input_idx=idx, dtype=RDT[prec], device=DEV)
    xg = x.to(CDT[prec]).to(DEV).requires_grad_(True)
    y = ops.filt_apply(xg, plan, layout=layout)
    gx, = torch.autograd.grad(y, xg, cot.to(CDT[prec]).to(DEV))
    return y.detach(), gx, plan, xg


def within(a, ref, scale, tol):
    err = (a.detach().cpu().to(torch.complex128) - ref).abs()
    bad = err > tol * scale
    assert not bool(bad.any()), 'worst error / scale %.3e at %d of %d elements' % (
        float((err / scale.clamp_min(1e-300))[bad].max()), int(bad.sum()), bad.numel())


# the residual of a rectangular filter is not defined (ops.filt_tables raises, as the reference does): no such case
KERNEL_CASES = [(n, m) for n in SHAPES for m in ('plain', 'residual', 'input_idx') if not (m == 'residual' and SHAPES[n][0] != SHAPES[n][1])]


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('cplx', [False, True], ids=['realG', 'complexG'])
@pytest.mark.parametrize('name,mode', KERNEL_CASES, ids=['%s-%s' % c for c in KERNEL_CASES])
def test_kernel_against_the_oracle(name, mode, cplx, prec):
    M, K, lead, Nbl, Nt, b2f = SHAPES[name]
    G, x, cot, idx = make_inputs(name, cplx, mode, prec)
    y64, sy, gx64, sg = oracle_filter(x, G, residual=(mode == 'residual'), input_idx=idx, bl2filt=b2f, cot=cot)
    y, gx, _, _ = run_gpu(G, x, cot, mode == 'residual', idx, (Nbl, Nt, b2f), prec)
    assert y.shape == y64.shape and gx.shape == x.shape and y.dtype == CDT[prec]
    within(y, y64, sy, TOL[prec])
    within(gx, gx64, sg, TOL[prec])
    if mode == 'input_idx':
        keep = np.setdiff1d(np.arange(K), idx)
        assert torch.equal(y[..., keep].cpu(), x[..., keep].to(CDT[prec]))           # unfiltered channels: the input's bits
    if min(b2f) < 0:
        un = [b for b, f in enumerate(b2f) if f < 0]
        assert torch.equal(y[..., un, :, :].cpu(), x[..., un, :, :].to(CDT[prec]))   # unassigned baselines pass through


@pytest.mark.parametrize('cplx', [False, True], ids=['realG', 'complexG'])
@pytest.mark.parametrize('mode', ['plain', 'residual', 'input_idx'])
def test_adjoint_identity(mode, cplx):
    """<W x, g> = <x, W^H g> in float64, for the operator of every mode"""
    name = 'N37_pol4_3filt'
    G, x, cot, idx = make_inputs(name, cplx, mode, 'f64')
    _, _, _, Nbl, Nt, b2f = SHAPES[name]
    y, gx, _, _ = run_gpu(G, x, cot, mode == 'residual', idx, (Nbl, Nt, b2f), 'f64')
    lhs = (y.cpu().conj() * cot).sum()
    rhs = (x.conj() * gx.cpu()).sum()
    assert abs(lhs - rhs) < 1e-12 * abs(lhs), (lhs, rhs)


@pytest.mark.parametrize('cplx', [False, True], ids=['realG', 'complexG'])
@pytest.mark.parametrize('mode', ['plain', 'residual', 'input_idx'])
def test_gradcheck(mode, cplx):
    from bayeslim_amd import ops
    rng = np.random.default_rng(9)
    K, M = 6, (4 if mode == 'input_idx' else 6)
    idx = [0, 2, 3, 5] if mode == 'input_idx' else None
    G = cnormal(rng, 2, M, K) if cplx else torch.as_tensor(rng.normal(size=(2, M, K)))
    plan = ops.FiltPlan(G, residual=(mode == 'residual'), input_idx=idx, dtype=torch.float64, device=DEV)
    x = cnormal(rng, 1, 3, 2, K).to(DEV).requires_grad_(True)
    fn = lambda t: ops.filt_apply(t, plan, layout=(3, 2, (1, -1, 0)))
    assert torch.autograd.gradcheck(fn, (x,), eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_bit_identity_run_to_run(prec):
    name = 'N64_3filt'
    G, x, cot, idx = make_inputs(name, True, 'residual', prec)
    _, _, _, Nbl, Nt, b2f = SHAPES[name]
    y1, g1, _, _ = run_gpu(G, x, cot, True, None, (Nbl, Nt, b2f), prec)
    y2, g2, _, _ = run_gpu(G, x, cot, True, None, (Nbl, Nt, b2f), prec)
    assert torch.equal(y1, y2) and torch.equal(g1, g2)


def test_plan_refuses_a_mismatch():
    from bayeslim_amd import ops
    G = torch.eye(4, dtype=torch.float64)
    plan = ops.FiltPlan(G, dtype=torch.float32, device=DEV)
    x = torch.zeros(3, 4, dtype=torch.complex64, device=DEV)
    with pytest.raises(TypeError):
        ops.filt_apply(x.to(torch.complex128), plan)
    with pytest.raises(ValueError):
        ops.filt_apply(x[:, :3], plan)
    with pytest.raises(ValueError):
        ops.filt_apply(x, plan, layout=(2, 1, (0, 0)))                     # 3 lines do not divide into 2 baselines
    with pytest.raises(ValueError):
        ops.filt_apply(x, plan, layout=(3, 1, (0, 1, 0)))                  # filter 1 of a one-filter plan
    with pytest.raises(RuntimeError):
        ops.filt_apply(x.cpu(), plan)
    rect = ops.FiltPlan(torch.ones(2, 4, dtype=torch.float64), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        ops.filt_apply(x, rect, layout=(3, 1, (0, -1, 0)))                 # a copied line would change its length
    # a real tensor is filtered as a complex one and comes back real under a real G
    xr = torch.arange(12, dtype=torch.float32, device=DEV).reshape(3, 4)
    assert torch.equal(ops.filt_apply(xr, plan), xr)


# --------------------------------------------------------------------------------------------------------------------
# the modules on the reference's vectors
# --------------------------------------------------------------------------------------------------------------------
def module_case(g, tag):
    from bayeslim_amd import filt
    if tag.startswith('mat_'):
        _, kind, res = tag.split('_')
        return filt.MatFilter(g['mat_G_' + kind], residual=(res == 'res1')), g['mat_x'], g['mat_G_' + kind], res == 'res1', None, -1
    if tag == 'rect':
        return filt.MatFilter(g['rect_G']), g['mat_x'], g['rect_G'], False, None, -1
    if tag.startswith('inp_'):
        res = tag.endswith('res1')
        return filt.MatFilter(g['inp_G'], residual=res, input_idx=g['inp_idx']), g['mat_x'], g['inp_G'], res, g['inp_idx'], -1
    assert tag == 'dim2'
    return filt.MatFilter(g['mat_G_cplx'], dim=-2, residual=True), g['dim2_x'], g['mat_G_cplx'], True, None, -2


MODULE_CASES = ['mat_real_res0', 'mat_real_res1', 'mat_cplx_res0', 'mat_cplx_res1', 'rect', 'inp_res0', 'inp_res1', 'dim2']


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('tag', MODULE_CASES)
def test_modules_on_the_reference_vectors(tag, prec):
    g = golden()
    f, x, G, res, idx, dim = module_case(g, tag)
    f.push(DEV)
    xg = x.to(CDT[prec]).to(DEV).requires_grad_(True)
    y = f(xg)
    (y.abs() ** 2).sum().backward()
    xo = x.movedim(dim, -1) if dim != -1 else x
    _, sy, _, _ = oracle_filter(xo, G, residual=res, input_idx=idx)
    sy = sy.movedim(-1, dim) if dim != -1 else sy
    # the stored vectors are float64.  In float32 the operands G and x are rounded first (relative eps / 2 each): every
    # product carries up to eps more than the arithmetic bound, and a sample the filter leaves untouched (scale 0: a column
    # outside input_idx) is a copy of the ROUNDED input, eps / 2 |x| from the stored one.  float64 rounds nothing.
    rnd = torch.finfo(torch.float32).eps if prec == 'f32' else 0.0
    out = g[tag + '_out']
    within(y, out, sy * (TOL[prec] + 2 * rnd) + torch.where(sy == 0, out.abs(), torch.zeros_like(sy)) * rnd, 1.0)
    ref = g[tag + '_grad']
    gtol = 1e-11 if prec == 'f64' else 1e-4
    assert float((xg.grad.cpu() - ref).abs().max() / ref.abs().max()) < gtol


def make_wedge(g):
    from bayeslim_amd import filt
    bls = [tuple(b) for b in g['wedge_bls'].tolist()]
    f2b = {0: [tuple(b) for b in g['wedge_bls0'].tolist()], 1: [tuple(b) for b in g['wedge_bls1'].tolist()]}
    members = [filt.MatFilter(g['mat_G_real'], residual=True), filt.MatFilter(g['mat_G_cplx'], residual=True)]
    return filt.WedgeFilter(members, f2b, bls=bls), bls


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_wedge_filter_tensor_and_visdata_one_launch_each_way(prec):
    from bayeslim_amd import ops, dataset
    g = golden()
    w, bls = make_wedge(g)
    w.push(DEV)
    xg = g['wedge_x'].to(CDT[prec]).to(DEV).requires_grad_(True)
    prof = []
    ops.PROFILE = prof
    try:
        y = w(xg)
        assert len(prof) == 1 and prof[0][0] == 'filt_kernel'              # both groups and the unassigned lines: one launch
        (y.abs() ** 2).sum().backward()
        assert len(prof) == 2
    finally:
        ops.PROFILE = None
    ref, gref = g['wedge_out'], g['wedge_grad']
    vtol, gtol = (1e-12, 1e-11) if prec == 'f64' else (1e-5, 1e-4)
    assert float((y.detach().cpu() - ref).abs().max() / ref.abs().max()) < vtol
    assert float((xg.grad.cpu() - gref).abs().max() / gref.abs().max()) < gtol
    un = [1, 4]
    assert torch.equal(y[..., un, :, :], xg[..., un, :, :])
    # the same data as a VisData with its baselines in another order than `bls`: the object's own baselines decide
    perm = [3, 0, 6, 1, 5, 2, 4]
    vd = dataset.VisData()
    vd.setup_data([bls[p] for p in perm], g['wedge_times'].numpy(), g['wedge_freqs'].to(DEV), pol='ee',
                  data=xg.detach()[:, :, perm].contiguous())
    out = w(vd)
    assert isinstance(out, dataset.VisData) and out is not vd and out.data is not vd.data and out.bls == vd.bls
    assert torch.equal(out.data, y.detach()[:, :, perm])
    assert torch.equal(vd.data, xg.detach()[:, :, perm])


def test_inplace_and_predict():
    from bayeslim_amd import filt
    g = golden()
    x = g['mat_x'].to(DEV)
    f = filt.MatFilter(g['mat_G_cplx'], residual=True, inplace=True)
    f.push(DEV)
    ref = filt.MatFilter(g['mat_G_cplx'].to(DEV), residual=True)(x)
    buf = x.clone()
    out = f(buf)
    assert out is buf and torch.equal(buf, ref) and not torch.equal(buf, x)
    pred = f.predict(x)                                                     # G x without the residual
    assert float((x - pred - ref).abs().max()) < 1e-13
    w, bls = make_wedge(g)
    w.inplace = True
    w.push(DEV)
    xv = g['wedge_x'].to(DEV)
    buf = xv.clone()
    assert w(buf) is buf and float((buf.cpu() - g['wedge_out']).abs().max()) < 1e-12
    # set_G_idx: a filter on a sub-band is the sub-block of G
    sub = filt.MatFilter(g['mat_G_cplx'].to(DEV))
    sub.set_G_idx(torch.arange(4, 12))
    y = sub(x[..., 4:12])
    want = torch.einsum('ij,abj->abi', g['mat_G_cplx'][4:12, 4:12], g['mat_x'][..., 4:12])
    assert float((y.cpu() - want).abs().max()) < 1e-13


def test_push_pickle_deepcopy_on_the_device():
    from bayeslim_amd import filt
    g = golden()
    w, bls = make_wedge(g)
    w.push(DEV)
    x64 = g['wedge_x'].to(DEV)
    y64 = w(x64)
    assert '_plans' in w.__dict__
    for cp in (pickle.loads(pickle.dumps(w)), copy.deepcopy(w)):
        assert '_plans' not in cp.__dict__ and cp.filters[0].G.is_cuda
        assert torch.equal(cp(x64), y64)                                     # the plan is rebuilt on first use
    y32 = w(x64.to(torch.complex64))                                         # another precision: another plan, same object
    assert y32.dtype == torch.complex64 and float((y32.cpu() - g['wedge_out']).abs().max() / g['wedge_out'].abs().max()) < 1e-5
    w.push(torch.float32)
    assert '_plans' not in w.__dict__ and w.filters[0].G.dtype == torch.float32 and w.filters[1].G.dtype == torch.complex64
    assert w(x64.to(torch.complex64)).dtype == torch.complex64
    gp = filt.GPFilter(g['gp_Cs'].clone(), g['gp_Cn'].clone(), residual=True)
    gp.push(DEV)
    x = g['mat_x'][..., :12].to(DEV)
    y = gp(x)
    gp.G = gp.G * 0.5                                                        # a new G: the stale plan must not be used
    want = x - torch.einsum('ij,abj->abi', gp.G.to(x.dtype), x)
    assert not torch.equal(gp(x), y) and float((gp(x) - want).abs().max()) < 1e-12


# --------------------------------------------------------------------------------------------------------------------
# RIME -> WedgeFilter in one Sequential
# --------------------------------------------------------------------------------------------------------------------
def test_sequential_rime_wedge_on_rime_c2_mini():
    """float32: visibilities = oracle filter of the golden visibilities (1e-5 of max); sky gradients = RIME's own backward
    fed with the oracle's adjoint of the cotangent (1e-4 of max)"""
    import bayeslim_amd
    from bayeslim_amd import filt, utils
    from conftest import load_golden
    import test_rime_gpu as trg
    g = load_golden('rime_c2_mini')
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    try:
        rime, sky, beam = trg._c2_setup(bayeslim_amd, g)
        bls = [tuple(b) for b in g['sim_bls'].tolist()]
        ants = g['ants'].tolist()
        pos = {a: v for a, v in zip(ants, g['antvecs'])}
        blen = np.array([np.linalg.norm(pos[b[1]] - pos[b[0]]) for b in bls])
        # three delay widths by baseline length; the longest baselines stay unfiltered
        edges = np.quantile(blen, [0.3, 0.6, 0.9])
        grp = np.searchsorted(edges, blen, side='right')
        f = torch.as_tensor(g['freqs'], dtype=torch.float64)
        fn = (f - f[0]) / (f[-1] - f[0])
        members = [filt.GPFilter(filt.sinc_cov(fn, ls), torch.eye(len(fn), dtype=torch.float64) * 1e-2, residual=True)
                   for ls in (1.5, 0.8, 0.4)]
        f2b = {i: [bl for bl, k in zip(bls, grp) if k == i] for i in range(3)}
        assert all(len(v) for v in f2b.values()) and (grp == 3).any()
        wedge = filt.WedgeFilter(members, f2b)
        wedge.push(torch.device(DEV))
        model = utils.Sequential({'rime': rime, 'wedge': wedge})
        out = model()
        b2f = tuple(int(k) if k < 3 else -1 for k in grp)
        Gs = torch.stack([m.G.cpu().to(torch.float64) for m in members])
        gw = torch.as_tensor(g['gvis'])
        y64, _, cot64, _ = oracle_filter(torch.as_tensor(g['vis']), Gs, residual=True, bl2filt=b2f, cot=gw)
        assert float((out.data.detach().cpu() - y64).abs().max() / y64.abs().max()) < 1e-5
        loss = (out.data * trg.T(g['gvis']).conj()).real.sum()
        grad, = torch.autograd.grad(loss, [sky.params])
        vis0 = rime().data
        want, = torch.autograd.grad((vis0 * cot64.to(torch.complex64).to(DEV).conj()).real.sum(), [sky.params])
        assert float((grad - want).abs().max() / want.abs().max()) < 1e-4
    finally:
        torch.set_default_dtype(old)
