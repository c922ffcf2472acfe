"""
GPU checks of the partly redundant inflation (csrc/partred.hip through ops.partred_inflate and
calibration.PartialRedVisInflate): the reference's fixture in complex128, the float64 restatement on float32-rounded inputs in
complex64, the edge shapes of the three kernels (each run twice, bit for bit), views as input, needs_input_grad, and the
module: default params, the gradient through p0 and R, priors, push, pickle / deepcopy, and a Sequential with RedVisAvg.
Every accuracy check asserts error / bound <= 1 per component with the derived bound of tests/partred_common.py.
"""
import copy
import pickle

import numpy as np
import pytest
import torch

import partred_common as pc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
RDT = {'f32': torch.float32, 'f64': torch.float64}


def npy(x):
    return x.detach().cpu().numpy()


def run(c, V, G, plan, prec, need=(True, True)):
    """(out, gV, gc) of ops.partred_inflate on the GPU with the cotangent G"""
    from bayeslim_amd import ops
    v = torch.as_tensor(V, dtype=CDT[prec], device=DEV).requires_grad_(need[0])
    cc = torch.as_tensor(c, dtype=RDT[prec], device=DEV).requires_grad_(need[1])
    out = ops.partred_inflate(v, cc, plan)
    if any(need):
        out.backward(torch.as_tensor(G, dtype=CDT[prec], device=DEV))
    return out.detach(), v.grad, cc.grad


def check(name, res, c, V, G, rows, cols, Nout, Nin, prec):
    """the three results against the restatement on the same (float32-exact) inputs"""
    out, gV, gc = pc.evaluate(c, V, rows, cols, Nout, G)
    Mo, Mv, Mc = pc.magnitudes(c, V, rows, cols, Nout, G)
    L = V.shape[0] * V.shape[1] * V.shape[3] * V.shape[4]
    n = pc.roundings(pc.build_plan(rows, cols, Nout, Nin), L, Nout, Nin)
    worst = dict(out=pc.ratio(npy(res[0]), out, pc.bound(Mo, n['kernel'][0], prec, n['numpy'][0])),
                 gV=pc.ratio(npy(res[1]), gV, pc.bound(Mv, n['kernel'][1], prec, n['numpy'][1])),
                 gc=pc.ratio(npy(res[2]), gc, pc.bound(Mc, n['kernel'][2], prec, n['numpy'][2])))
    print(name, prec, 'worst error / bound:', worst)
    assert max(worst.values()) <= 1.0, worst
    return out, gV, gc


def visdata(data, bls, Nt, Nf):
    from bayeslim_amd import dataset, utils
    vd = dataset.VisData()
    vd.setup_meta(None, utils.AntposDict(pc.ANTS, pc.ANTVECS))
    vd.setup_data(bls, torch.arange(float(Nt)), torch.linspace(1e8, 2e8, Nf), pol='ee' if data.shape[0] == 1 else None, data=data)
    return vd


IN_BLS = [(a, a) for a in pc.ANTS] + [(0, 1), (0, 2)]


def fixture_module(name, dtype):
    from bayeslim_amd import calibration as cal
    g, case = pc.golden(), pc.GOLDEN_CASES[name]
    m = cal.PartialRedVisInflate(dict(zip(case['new_bls'], case['lists'])), list(case['new_bls']),
                                 params=torch.as_tensor(g['params_' + name]).to(dtype),
                                 p0=torch.as_tensor(g['p0_' + name]).to(dtype) if case['p0'] else None,
                                 R=getattr(torch, case['R']) if case['R'] else None)
    m.push(DEV)
    return m


@pytest.mark.parametrize('name', list(pc.GOLDEN_CASES))
def test_fixture_in_complex128_through_the_module(name):
    """module forward and the gradients of sum w |out|^2 against the reference's record; the cotangent comes from the output:
    its roundings are added, and those of the chain rule through R for params (module docstring of partred_common)"""
    g, case = pc.golden(), pc.GOLDEN_CASES[name]
    rows, cols, _ = pc.entry_list(case['lists'])
    Nout, Nin = (int(x) for x in g['Ashape_' + name])
    m = fixture_module(name, torch.float64)
    d = torch.as_tensor(g['data_' + name], device=DEV).requires_grad_(True)
    w = torch.as_tensor(g['w_' + name], device=DEV)
    vout = m(visdata(d, IN_BLS[:Nin], pc.NT, pc.NF))
    assert vout.bls == list(case['new_bls']) and tuple(vout.data.shape) == tuple(g['V_' + name].shape)
    ((vout.data.real ** 2 + vout.data.imag ** 2) * w).sum().backward()
    R, dR = pc.RESPONSES[case['R']]
    x = g['params_' + name] + (g['p0_' + name] if case['p0'] else 0.0)
    c, V = R(x), g['data_' + name]
    L = V.shape[0] * V.shape[1] * V.shape[3] * V.shape[4]
    n = pc.roundings(pc.build_plan(rows, cols, Nout, Nin), L, Nout, Nin)
    Mo, _, _ = pc.magnitudes(c, V, rows, cols, Nout)
    _, Mv, Mc = pc.magnitudes(c, V, rows, cols, Nout, G=2 * g['w_' + name] * Mo)
    fwd = n['kernel'][0] + n['fixture'][0] + 2 + pc.CHAIN                   # c = R(params + p0) is evaluated by either side
    worst = dict(out=pc.ratio(npy(vout.data), g['V_' + name], pc.bound(Mo, n['kernel'][0], 'f64', n['fixture'][0], extra=pc.CHAIN)),
                 gd=pc.ratio(npy(d.grad), g['gd_' + name], pc.bound(Mv, n['kernel'][1], 'f64', n['fixture'][1], extra=fwd)),
                 gp=pc.ratio(npy(m.params.grad), g['gp_' + name],
                             pc.bound(Mc * np.abs(dR(x)), n['kernel'][2], 'f64', n['fixture'][2], extra=fwd + pc.CHAIN)))
    print(name, 'f64 against the fixture, worst error / bound:', worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('name', list(pc.GOLDEN_CASES))
def test_fixture_cases_in_complex64_against_the_restatement(name):
    from bayeslim_amd import ops
    g, case = pc.golden(), pc.GOLDEN_CASES[name]
    rows, cols, _ = pc.entry_list(case['lists'])
    Nout, Nin = (int(x) for x in g['Ashape_' + name])
    R, _ = pc.RESPONSES[case['R']]
    f32 = lambda a, t: np.asarray(a).astype(t).astype(np.complex128 if t == np.complex64 else np.float64)
    c = f32(R(g['params_' + name] + (g['p0_' + name] if case['p0'] else 0.0)), np.float32)
    V = f32(g['data_' + name], np.complex64)
    G = f32(2 * g['w_' + name] * g['V_' + name], np.complex64)
    plan = ops.PartRedPlan(rows, cols, Nout, Nin)
    check(name, run(c, V, G, plan, 'f32'), c, V, G, rows, cols, Nout, Nin, 'f32')


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('name', list(pc.KERNEL_CASES))
def test_edge_shapes_twice_bit_for_bit(name, prec):
    from bayeslim_amd import ops
    case = pc.KERNEL_CASES[name]
    lists = pc.case_lists(case)
    rows, cols, _ = pc.entry_list(lists)
    Nout, Nin = len(lists), case['Nin']
    plan = ops.PartRedPlan(rows, cols, Nout, Nin)
    c, V, G = pc.case_arrays(name, case['Npol'], Nin, Nout, len(rows), case['Nt'], case['Nf'])
    a, b = run(c, V, G, plan, prec), run(c, V, G, plan, prec)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    check(name, a, c, V, G, rows, cols, Nout, Nin, prec)
    for i, red in enumerate(lists):
        if not isinstance(red, int) and len(red) == 0:
            assert float(a[0][:, :, i].abs().max()) == 0.0                   # a row without entries: exactly 0
    for j in set(range(Nin)) - set(cols.tolist()):
        assert float(a[1][:, :, j].abs().max()) == 0.0                       # a column without entries: exactly 0
    if name == 'long_row':
        assert plan.max_row == pc.ECH + 1
    if name == 'long_col':
        assert plan.max_col > pc.WAVES * pc.UNROLL


@pytest.mark.parametrize('view', ['moveaxis', 'expand', 'slice_p2'])
def test_views_are_read_in_place(view):
    from bayeslim_amd import ops
    case = pc.KERNEL_CASES['f67' if view == 'expand' else 'empty_col']           # the 2-pol case where the pol axes matter
    lists = pc.case_lists(case)
    rows, cols, _ = pc.entry_list(lists)
    Nout, Nin, NP, Nt, Nf = len(lists), case['Nin'], case['Npol'], case['Nt'], case['Nf']
    plan = ops.PartRedPlan(rows, cols, Nout, Nin)
    c, V, G = pc.case_arrays(view, NP, Nin, Nout, len(rows), Nt, Nf)
    cc = torch.as_tensor(c, dtype=torch.float32, device=DEV).requires_grad_(True)
    if view == 'moveaxis':                                                    # the baseline axis in front, as the reference lays it out
        base = torch.as_tensor(np.moveaxis(V, 2, 0).copy(), dtype=torch.complex64, device=DEV).requires_grad_(True)
        v = base.moveaxis(0, 2)
        assert not v.is_contiguous()
    elif view == 'expand':                                                    # one time for all
        V = np.broadcast_to(V[:, :, :, :1], V.shape).copy()
        base = torch.as_tensor(V[:, :, :, :1], dtype=torch.complex64, device=DEV).requires_grad_(True)
        v = base.expand(NP, NP, Nin, Nt, Nf)
        assert v.stride(3) == 0
    else:                                                                     # every other channel of a wider 2-pol tensor
        wide = np.zeros(V.shape[:4] + (2 * Nf,), dtype=np.complex128)
        wide[..., ::2] = V
        base = torch.as_tensor(wide, dtype=torch.complex64, device=DEV).requires_grad_(True)
        v = base[..., ::2]
        assert v.stride(4) == 2
    out = ops.partred_inflate(v, cc, plan)
    out.backward(torch.as_tensor(G, dtype=torch.complex64, device=DEV))
    ref = run(c, V, G, plan, 'f32')                                           # the same values as a contiguous tensor
    assert torch.equal(out.detach(), ref[0]) and torch.equal(cc.grad, ref[2])
    if view == 'moveaxis':
        assert torch.equal(base.grad.moveaxis(0, 2), ref[1])
    elif view == 'slice_p2':
        assert torch.equal(base.grad[..., ::2], ref[1]) and float(base.grad[..., 1::2].abs().max()) == 0.0
    else:
        assert tuple(base.grad.shape) == (NP, NP, Nin, 1, Nf) and Nt == 2        # the sum of two numbers rounds once
        assert torch.equal(base.grad[:, :, :, 0], ref[1][:, :, :, 0] + ref[1][:, :, :, 1])
    check(view, ref, c, V, G, rows, cols, Nout, Nin, 'f32')


def test_gradients_only_where_asked():
    from bayeslim_amd import ops
    case = pc.KERNEL_CASES['f67']
    lists = pc.case_lists(case)
    rows, cols, _ = pc.entry_list(lists)
    Nout, Nin = len(lists), case['Nin']
    plan = ops.PartRedPlan(rows, cols, Nout, Nin)
    c, V, G = pc.case_arrays('f67', 1, Nin, Nout, len(rows), case['Nt'], case['Nf'])
    both = run(c, V, G, plan, 'f32')
    data_only = run(c, V, G, plan, 'f32', need=(True, False))
    coeff_only = run(c, V, G, plan, 'f32', need=(False, True))
    assert data_only[2] is None and torch.equal(data_only[1], both[1]) and torch.equal(data_only[0], both[0])
    assert coeff_only[1] is None and torch.equal(coeff_only[2], both[2])
    none = run(c, V, G, plan, 'f32', need=(False, False))
    assert none[1] is None and none[2] is None and torch.equal(none[0], both[0])
    with pytest.raises(ValueError, match='columns'):
        ops.partred_inflate(torch.zeros(1, 1, Nin + 1, 2, 3, dtype=torch.complex64, device=DEV), torch.ones(len(rows), device=DEV), plan)
    with pytest.raises(ValueError, match='coeff'):
        ops.partred_inflate(torch.zeros(1, 1, Nin, 2, 3, dtype=torch.complex64, device=DEV), torch.ones(len(rows) + 1, device=DEV), plan)


def test_default_params_average_the_contributing_models():
    from bayeslim_amd import calibration as cal
    case = pc.GOLDEN_CASES['p1_sorted']
    m = cal.PartialRedVisInflate(dict(zip(case['new_bls'], case['lists'])), list(case['new_bls']))
    m.push(DEV)
    assert m.device == DEV and m.idx.is_cuda and m.Nred.is_cuda and m.params.is_cuda and isinstance(m.params, torch.nn.Parameter)
    _, V, _ = pc.case_arrays('avg', 1, 5, 6, 12, pc.NT, pc.NF)
    d = torch.as_tensor(V, dtype=torch.complex64, device=DEV)
    out = m(visdata(d, IN_BLS[:5], pc.NT, pc.NF)).data
    assert out.dtype == torch.complex64
    for i, red in enumerate(case['lists']):
        assert torch.allclose(out[:, :, i], d[:, :, red].mean(2), rtol=1e-6, atol=1e-6)


def test_gradient_reaches_params_through_p0_and_R_and_priors_are_filled():
    """central finite difference of sum w |out|^2 in float64 (step h, error O(h^2) of the third derivative: 1e-6 relative with
    h = 1e-4 on O(1) values) against the analytic gradient"""
    g, name = pc.golden(), 'p1_exp'
    m = fixture_module(name, torch.float64)
    Nin = int(g['Ashape_' + name][1])
    d = torch.as_tensor(g['data_' + name], device=DEV)
    w = torch.as_tensor(g['w_' + name], device=DEV)
    vd = visdata(d, IN_BLS[:Nin], pc.NT, pc.NF)
    seen = []

    class Prior:
        def __call__(self, p):
            seen.append(p.detach().clone())
            return (p ** 2).sum()

        def push(self, device):
            pass

    m.set_priors(priors_inp_params=Prior(), priors_out_params=Prior())
    def loss():
        o = m(vd).data.detach()
        return float(((o.real ** 2 + o.imag ** 2) * w).sum())

    cache = {}
    out = m(vd, prior_cache=cache).data
    ((out.real ** 2 + out.imag ** 2) * w).sum().backward()
    assert list(cache) == [m.name] and len(seen) == 2
    assert torch.equal(seen[0], m.params.detach()) and torch.equal(seen[1], torch.exp(m.params.detach() + m.p0))
    assert float(cache[m.name].detach()) == pytest.approx(float((seen[0] ** 2).sum() + (seen[1] ** 2).sum()))
    grad, h = m.params.grad.clone(), 1e-4
    for k in (0, 3, 10):
        with torch.no_grad():
            m.params[k] += h
            up = loss()
            m.params[k] -= 2 * h
            dn = loss()
            m.params[k] += h
        fd = (up - dn) / (2 * h)
        assert abs(fd - float(grad[k])) <= 1e-5 * max(abs(fd), 1.0), (k, fd, float(grad[k]))


def test_push_to_a_dtype_pickle_and_deepcopy_after_a_forward():
    g, name = pc.golden(), 'p1_exp'
    m = fixture_module(name, torch.float64)
    Nin = int(g['Ashape_' + name][1])
    d = torch.as_tensor(g['data_' + name], device=DEV)
    vd = visdata(d, IN_BLS[:Nin], pc.NT, pc.NF)
    out = m(vd).data
    assert out.dtype == torch.complex128 and out.requires_grad
    for q in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert '_tabs' not in q.plan.__dict__ and q.params.is_cuda
        assert torch.equal(q(vd).data, out)
    m.push(torch.float32)
    assert m.params.dtype == torch.float32 and m.p0.dtype == torch.float32 and m.idx.dtype == torch.int64
    out32 = m(visdata(d.to(torch.complex64), IN_BLS[:Nin], pc.NT, pc.NF)).data
    assert out32.dtype == torch.complex64 and torch.allclose(out32, out.to(torch.complex64), rtol=1e-5, atol=1e-5)
    assert m(vd).data.dtype == torch.complex128                               # c is cast to the real dtype of the data


def test_sequential_of_average_and_inflation():
    from bayeslim_amd import calibration as cal, dataset, utils
    from collections import OrderedDict
    bls = [(0, 1), (1, 2), (0, 2), (2, 3), (1, 3)]
    reds = [[(0, 1), (1, 2), (2, 3)], [(0, 2), (1, 3)]]
    bl2red = {(0, 1): 0, (1, 2): [0, 1], (0, 2): 1, (2, 3): [1, 0], (1, 3): [1]}
    _, V, _ = pc.case_arrays('seq', 1, 5, 5, 7, 2, 67)
    d = torch.as_tensor(V, dtype=torch.complex64, device=DEV)
    vd = visdata(d, bls, 2, 67)
    infl = cal.PartialRedVisInflate(bl2red, bls)
    seq = utils.Sequential(OrderedDict(avg=dataset.RedVisAvg(reds), inflate=infl))
    seq.push(DEV)
    cache = {}
    vout = seq(vd, prior_cache=cache)
    assert vout.bls == bls and tuple(vout.data.shape) == (1, 1, 5, 2, 67) and torch.equal(vout.times, vd.times)
    avg = vd.bl_average(reds=reds).data
    assert avg.shape[2] == 2 == infl.Ashape[1]
    assert torch.allclose(vout.data[0, 0, 0], avg[0, 0, 0]) and torch.allclose(vout.data[0, 0, 3], avg[0, 0].mean(0), rtol=1e-6, atol=1e-6)
    vout.data.abs().sum().backward()
    assert infl.params.grad is not None and bool(infl.params.grad.abs().sum() > 0)
