#!/usr/bin/env python3
"""
Golden vectors of the partly redundant inflation (reference calibration.py: PartialRedVisInflate :2178-2344) on the CPU in
float64 / complex128, 3 times, 5 channels.  TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes
tests/golden/partred.npz (arrays only).

Recorded per case of partred_common.GOLDEN_CASES (1-pol with sorted lists of 1 to 3 entries and the default params; 2-pol with
unsorted lists and plain integers as values of bl2red; one case with p0 and R = torch.exp, named in the fixture as R_<case>):
idx, Nred, Ashape, params, p0 (where set), the input data, fixed weights w, the output and the gradients of sum w |out|^2
with respect to params and to the data.  Every case is recorded with use_csr=False, the defining path (params[k] belongs to
entry idx[:, k]).  The values of bl2red are Python ints or lists: the reference tests `isinstance(red, int)`, so a numpy
integer fails there (len() of a scalar); the product accepts both.

torch.sparse.mm on a CSR matrix does run on the CPU here: the sorted case 'p1_sorted' is also run with use_csr=True and
asserted to agree with the dense path to 1e-12 (output and both gradients); it is recorded as csr_ran = 1.  With unsorted
lists the reference's CSR path assigns params to other entries (to_sparse_csr sorts the columns of a row); checked here too
(csr_unsorted_differs = 1) and not reproduced by the product.

Usage:  python tests/golden/make_golden_partred.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg            # noqa: E402
import partred_common as pc         # noqa: E402


def run(ba, cal, case, arrs, use_csr):
    antpos = {a: torch.as_tensor(v) for a, v in zip(pc.ANTS, pc.ANTVECS)}
    bl2red = dict(zip(case['new_bls'], case['lists']))
    params = None if arrs['params'] is None else arrs['params'].clone()
    p0 = None if arrs['p0'] is None else arrs['p0'].clone()
    m = cal.PartialRedVisInflate(bl2red, list(case['new_bls']), params=params, p0=p0,
                                 R=getattr(torch, case['R']) if case['R'] else None, use_csr=use_csr)
    Nin = m.Ashape[1]
    vd = ba.dataset.VisData()
    vd.setup_meta(None, antpos)
    d = arrs['data'].clone().requires_grad_(True)
    in_bls = [(a, a) for a in pc.ANTS] + [(0, 1), (0, 2)]           # names for the Nin model rows; never looked at
    vd.setup_data(in_bls[:Nin], arrs['times'], arrs['freqs'], pol='ee' if case['Npol'] == 1 else None, data=d)
    vout = m(vd)
    assert list(vout.bls) == list(case['new_bls']) and vout.data.shape[2] == len(case['new_bls'])
    ((vout.data.real ** 2 + vout.data.imag ** 2) * arrs['w']).sum().backward()
    return m, vout.data.detach(), m.params.grad.clone(), d.grad.clone()


def gen(ba):
    cal = mg.load_calibration_module(ba)
    rng = np.random.default_rng(2178)
    Nt, Nf = pc.NT, pc.NF
    freqs = torch.linspace(120e6, 180e6, Nf)
    times = torch.as_tensor(2459861.0 + np.arange(Nt) * 10.0 / 1440)
    out = dict(freqs=freqs, times=times)
    for tag, case in pc.GOLDEN_CASES.items():
        rows, cols, Nred = pc.entry_list(case['lists'])
        Nout, Nin, NP = len(case['new_bls']), int(cols.max()) + 1, case['Npol']
        cx = lambda *shape: torch.as_tensor(rng.normal(size=shape) + 1j * rng.normal(size=shape))
        arrs = dict(times=times, freqs=freqs, data=cx(NP, NP, Nin, Nt, Nf),
                    w=torch.as_tensor(rng.uniform(0.5, 2.0, size=(NP, NP, Nout, Nt, Nf))),
                    params=torch.as_tensor(rng.uniform(-0.8, 0.8, size=len(rows))) if case['params'] else None,
                    p0=torch.as_tensor(rng.uniform(-0.3, 0.3, size=len(rows))) if case['p0'] else None)
        m, V, gp, gd = run(ba, cal, case, arrs, use_csr=False)
        assert tuple(m.Ashape) == (Nout, Nin) and (m.idx.numpy() == np.stack([rows, cols])).all() and (m.Nred.numpy() == Nred).all()
        out.update({'idx_' + tag: m.idx, 'Nred_' + tag: m.Nred, 'Ashape_' + tag: np.array(m.Ashape), 'params_' + tag: m.params.detach(),
                    'data_' + tag: arrs['data'], 'w_' + tag: arrs['w'], 'V_' + tag: V, 'gp_' + tag: gp, 'gd_' + tag: gd,
                    'R_' + tag: np.array(case['R'] or 'identity')})
        if case['p0']:
            out['p0_' + tag] = arrs['p0']
        m2, V2, gp2, gd2 = run(ba, cal, case, arrs, use_csr=True)
        diff = max(float((V2 - V).abs().max()), float((gp2 - gp).abs().max()), float((gd2 - gd).abs().max()))
        is_sorted = all(list(r) == sorted(r) for r in case['lists'] if not isinstance(r, int))
        if tag == 'p1_sorted':
            assert is_sorted and diff < 1e-12, diff
            out['csr_ran'] = np.array(1)
        elif tag == 'p2_unsorted':
            assert not is_sorted
            out['csr_unsorted_differs'] = np.array(int(diff > 1e-3))
        print('%-12s Nout %d Nin %d Nnz %d   csr path - dense path: %.2e' % (tag, Nout, Nin, len(rows), diff))
    mg.save('partred', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen(mg.bootstrap_reference())
