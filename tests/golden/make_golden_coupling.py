#!/usr/bin/env python3
"""
Golden vectors of the mutual-coupling module (reference calibration.py: VisCoupling :1258-1586) on a 7-antenna hexagon plus
one outrigger, with `antpos` NOT in ascending antenna number, all ant2 >= ant1 baselines minus two cross baselines and one
auto-correlation (so the matrix has nulls), 3 times, 5 channels, float64 / complex128.  TEST INFRASTRUCTURE ONLY, like
make_golden.py, whose bootstrap it reuses; writes tests/golden/coupling.npz, arrays only.

Recorded: the index attributes of setup_coupling, `dly` for conj True / False with and without min_dly, and for every case of
GOLDEN_RECORDED the output and the gradients of sum w |W|^2 (fixed random weights w) with respect to params (real view) and
to vd.data.  float64 outputs of the full product of (prod, add_I, double, time axis) alone would exceed the size the fixture
may have, so the recorded cases are a covering table: every value of every keyword occurs, the two-sided product and `double`
with and without the identity and with both kinds of time axis.  Absent from the fixture, and checked against the numpy
restatement only (tests/test_coupling_gpu.py, case n8_dbl_tb): prod='left' with double=True and prod='left' with
add_I=False; their 'right' siblings are recorded.

Finding (reference): forward multiplies the output of the response by dly IN PLACE (:1501); with the default response and
parameters that require a gradient that output is a view of a leaf, and torch refuses.  The fixture gives the module a p0
of zeros, which makes the response input a fresh tensor (the documented use of p0).
Finding (reference): with double=True forward adds the second-order term to the coupling matrix IN PLACE (:1507), after
einsum has saved that matrix for its backward pass: the forward runs, backward raises.  The gradients of the double cases
are recorded from the module's own source with that one statement spelled out of place (`coupling = coupling + ...`,
substituted at generation time as load_calibration_module substitutes the py>=3.11 token), after checking that the
unmodified module gives the same output bit for bit.
Finding (reference): `double` of forward defaults to False, not None, so self.double is never consulted (:1505); the fixture
passes the keyword.

Usage:  python tests/golden/make_golden_coupling.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg        # noqa: E402
import coupling_common as cc    # noqa: E402

GOLDEN_RECORDED = ['both_I_sgl_pt', 'both_noI_dbl_tb', 'left_I_sgl_tb', 'right_noI_sgl_tb', 'right_I_dbl_pt']


IN_PLACE = 'coupling += torch.einsum'         # the one in-place statement of that kind in the module


def load_out_of_place(ba):
    """the reference's calibration module with the in-place second-order add of VisCoupling.forward spelled out of place"""
    import types
    src = open(os.path.join(mg.REF, 'calibration.py')).read().replace('[*self.idx]', '[tuple(self.idx)]')
    assert src.count(IN_PLACE) == 1
    src = src.replace(IN_PLACE, IN_PLACE.replace('coupling +=', 'coupling = coupling +'))
    mod = types.ModuleType('bayeslim.calibration_oop')
    mod.__package__ = 'bayeslim'
    mod.__file__ = os.path.join(mg.REF, 'calibration.py')
    exec(compile(src, mod.__file__, 'exec'), mod.__dict__)
    return mod


def gen_coupling(ba):
    cal = mg.load_calibration_module(ba)
    cal_oop = load_out_of_place(ba)
    rng = np.random.default_rng(1258)
    Nt, Nf = cc.NT, cc.NF
    freqs = torch.linspace(120e6, 180e6, Nf)
    times = torch.as_tensor(2459861.0 + np.arange(Nt) * 10.0 / 1440)
    arr = mg.hex_array(ba, 2, freqs)
    hex_ants, hex_vecs = list(arr.ants), np.asarray(arr.antvecs)
    assert len(hex_ants) == 7
    ants = hex_ants + [max(hex_ants) + 4]
    vecs = np.concatenate([hex_vecs, [[60.0, -25.0, 0.5]]])
    order = [5, 2, 7, 0, 3, 6, 1, 4]                      # the matrix order: not ascending in antenna number
    ants, vecs = [ants[k] for k in order], vecs[order]
    assert ants != sorted(ants)
    antpos = {a: torch.as_tensor(v) for a, v in zip(ants, vecs)}
    N = len(ants)
    s = sorted(ants)
    bls = [(a, b) for a in s for b in s if b >= a]
    for drop in [(s[0], s[3]), (s[2], s[7]), (s[4], s[4])]:
        bls.remove(drop)
    bls = [bls[k] for k in rng.permutation(len(bls))]
    Nbl = len(bls)

    def cx(*shape):
        return torch.as_tensor(rng.normal(size=shape) + 1j * rng.normal(size=shape))

    data = cx(1, 1, Nbl, Nt, Nf)
    w = torch.as_tensor(rng.uniform(0.5, 2.0, size=(1, 1, Nbl, Nt, Nf)))
    p_pt = 0.3 * torch.as_tensor(rng.normal(size=(1, 1, N, N, Nt, Nf, 2)))
    p_tb = 0.3 * torch.as_tensor(rng.normal(size=(1, 1, N, N, 1, Nf, 2)))
    out = dict(freqs=freqs, times=times, ants=np.array(ants), antvecs=vecs, bls=np.array(bls), data=data, w=w, p_pt=p_pt, p_tb=p_tb)

    def model(p, cal=cal):
        R = cal.VisModelResponse(param_type='com', times=times if p.shape[-3] > 1 else None)
        m = cal.VisCoupling(p.clone(), freqs, antpos, list(bls), R=R, p0=torch.zeros_like(p))
        return m

    m = model(p_pt)
    for tag, kw in (('ct', dict(conj=True)), ('cf', dict(conj=False)), ('ct_min', dict(conj=True, min_dly=20.0)),
                    ('cf_min', dict(conj=False, min_dly=20.0))):
        m.setup_coupling(**kw)
        out['dly_' + tag] = m.dly.clone()
    m.setup_coupling()
    for k in ('flat_data_idx', 'flat_conj_idx', 'flat_unconj_idx', 'flat_data_null', 'bls_idx', 'I'):
        out[k] = getattr(m, k)

    for tag in GOLDEN_RECORDED:
        kw = cc.GOLDEN_CASES[tag]
        m = model(p_tb if kw['tb'] else p_pt, cal_oop if kw['double'] else cal)
        m.setup_coupling()
        vd = ba.dataset.VisData()
        vd.setup_meta(None, antpos)
        d = data.clone().requires_grad_(True)
        vd.setup_data(bls, times, freqs, pol='ee', data=d)
        vout = m(vd, add_I=kw['add_I'], prod=kw['prod'], double=kw['double'])
        if kw['double']:
            m0 = model(p_tb if kw['tb'] else p_pt)
            m0.setup_coupling()
            vd0 = ba.dataset.VisData()
            vd0.setup_meta(None, antpos)
            vd0.setup_data(bls, times, freqs, pol='ee', data=data.clone())
            with torch.no_grad():
                assert torch.equal(m0(vd0, add_I=kw['add_I'], prod=kw['prod'], double=True).data, vout.data.detach())
        ((vout.data.real ** 2 + vout.data.imag ** 2) * w).sum().backward()
        out.update({'W_' + tag: vout.data.detach(), 'gp_' + tag: m.params.grad.clone(), 'gd_' + tag: d.grad.clone()})
    mg.save('coupling', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen_coupling(mg.bootstrap_reference())
