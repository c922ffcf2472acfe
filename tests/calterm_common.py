"""
Shared by tests/test_calibration_base.py and the deepcopy tests of tests/test_redcal_gpu.py, tests/test_coupling_gpu.py and
tests/test_redcoupling_gpu.py: the five calibration terms on the 7-antenna hexagon with 2 times and 3 channels -- the smallest
array on which every index table (redundant groups, matrix table, coupling entries) has more than one group and a conjugated
entry -- and the check that a deep copy taken after a forward and a backward computes what the original does.
"""
import copy

import numpy as np
import torch

from bayeslim_amd import calibration as cal, dataset, telescope_model, utils

NT, NF = 2, 3
CLASSES = ('JonesModel', 'RedVisModel', 'VisModel', 'VisCoupling', 'RedVisCoupling')


def hex7():
    """(antpos, all baselines with ant2 >= ant1, one baseline per redundant group, baseline -> group, times, freqs)"""
    ants, vecs = utils._make_hex(2, D=14.6)
    antpos = utils.AntposDict(ants, vecs)
    reds, _, bl2red, bls = telescope_model.build_reds(antpos)[:4]
    times = torch.as_tensor(2459861.0 + np.arange(NT) * 10.0 / 1440)
    freqs = torch.linspace(120e6, 130e6, NF, dtype=torch.float64)
    return antpos, [tuple(b) for b in bls], [tuple(r[0]) for r in reds], {tuple(k): int(v) for k, v in bl2red.items()}, times, freqs


def build(name, device='cpu', R=None, p0=False, seed=0, setup=True):
    """(module, input VisData) of the class `name` in float64 on `device`; R: the response (default: the class's own 'com'
    response that knows the times); p0: also give a p0 of the parameters' shape"""
    antpos, bls, bls_red, bl2red, times, freqs = hex7()
    rng = np.random.default_rng(seed)
    rnd = lambda *s: torch.as_tensor(rng.normal(size=s + (2,))).to(device)
    Nant, Nbl, Nred = len(antpos), len(bls), len(bls_red)
    kw = lambda p: dict(p0=0.1 * rnd(*p.shape[:-1]) if p0 else None)
    bls_in = bls
    if name == 'JonesModel':
        p = 0.3 * rnd(1, 1, Nant, NT, NF)
        p[..., 0] += 1
        m = cal.JonesModel(p, list(antpos.keys()), R=R or cal.JonesResponse(param_type='com', times=times, device=device), **kw(p))
    elif name == 'RedVisModel':
        p = rnd(1, 1, Nred, NT, NF)
        m = cal.RedVisModel(p, bl2red, R=R or cal.VisModelResponse(param_type='com', times=times, device=device), **kw(p))
    elif name == 'VisModel':
        p = rnd(1, 1, Nbl, NT, NF)
        m = cal.VisModel(p, R=R or cal.VisModelResponse(param_type='com', times=times, device=device),
                         blnums=torch.as_tensor(utils.ants2blnum(bls)), **kw(p))
    elif name == 'VisCoupling':
        p = 0.05 * rnd(1, 1, Nant, Nant, NT, NF)
        m = cal.VisCoupling(p, freqs.to(device), antpos, bls,
                            R=R or cal.VisModelResponse(param_type='com', times=times, device=device), **kw(p))
        if setup:
            m.setup_coupling(min_dly=2.0)
    elif name == 'RedVisCoupling':
        terms, idx = cal.gen_coupling_terms(antpos, compress_to_red=True)
        p = 0.05 * rnd(1, 1, len(terms), NT, NF)
        m = cal.RedVisCoupling(p, freqs.to(device), antpos, terms, bls_red, bls, coupling_idx=idx,
                               R=R or cal.VisModelResponse(param_type='com', times=times, device=device), **kw(p))
        if setup:
            m.setup_coupling(min_dly=2.0)
        bls_in = bls_red
    else:
        raise KeyError(name)
    vd = dataset.VisData()
    vd.setup_meta(None, antpos)
    data = rnd(1, 1, len(bls_in), NT, NF)
    vd.setup_data(bls_in, times, freqs, pol='ee', data=torch.view_as_complex(data))
    return m, vd


def check_deepcopy_after_backward(name, device):
    """forward and backward, then copy.deepcopy: the copy holds no cached output, its next forward is bit-equal to the
    original's, and the original's cached output is untouched by the copy"""
    m, vd = build(name, device=device)
    out = m(vd)
    (out.data.real ** 2 + out.data.imag ** 2).sum().backward()
    assert m.params.grad is not None and float(m.params.grad.abs().max()) > 0
    kept, kept_data = m._vd, m._vd.data
    other = copy.deepcopy(m)
    assert other._vd is None
    assert m._vd is kept and m._vd.data is kept_data
    want = m(vd).data.detach().clone()
    got = other(vd).data.detach()
    assert got.shape == want.shape and torch.equal(got, want)
    assert other._vd is not None and other._vd is not m._vd and m._vd is kept
    assert torch.equal(other.params.detach(), m.params.detach()) and other.params is not m.params
