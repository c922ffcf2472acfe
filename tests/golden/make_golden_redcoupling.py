#!/usr/bin/env python3
"""
Golden vectors of the redundant mutual-coupling module (reference calibration.py: RedVisCoupling :1588-2115, CouplingInflate
:2118-2175, configure_coupling_matrix_singlepath, gen_coupling_terms, cut_bl :3047-3400) on the 7-antenna hexagon plus one
outrigger of the coupling fixture, `antpos` NOT in ascending antenna number, every ant2 >= ant1 baseline (autos included) as
output, 3 times, 5 channels, float64 / complex128.  TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses;
writes tests/golden/redcoupling.npz (arrays only) and tests/golden/redcoupling_arows.json (the recorded Arows names).

Recorded per case of redcoupling_common.GOLDEN_CASES (a covering table of use_reds x compress_to_red x include_second_order x
time axis, plus one case with max_len / second_max_len cuts and no_auto_coupling terms): coupling_terms and coupling_idx, the
six index tuples, red_bl_inds, dly, get_coupling_hits, the output and the gradients of sum w |Vc|^2 (fixed random weights)
with respect to params (real view) and to the input data.  Also gen_coupling_terms with `ants=`, and CouplingInflate.idx / zeros.

Finding (reference): with use_reds=False and copydata=False forward adds to the input tensor IN PLACE (`vout.data +=`, :2011)
after einsum saved it, and the conjugated block then reads the already modified input; with parameters that need a gradient
torch refuses.  The physical-baseline cases are therefore recorded with copydata=True.  That copy is detached (VisData.copy), so
the reference's gradient of the data lacks the zeroth-order (identity) term; the fixture adds it back (gd += the cotangent
2 w Vc, rows and columns coincide) and says so here.
Finding (reference): the module is given a p0 of zeros as in the coupling fixture, so that the response input is a fresh tensor.
Checked at generation: no first-order index tuple holds the same (row, column) twice (torch's indexed `+=` would keep one of
the two where the entry list sums them).

Usage:  python tests/golden/make_golden_redcoupling.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg            # noqa: E402
import redcoupling_common as rc     # noqa: E402

AROWS_RECORDED = ['cuts', 'red_all_fo_tb', 'phys_cmp_fo_pt', 'red_cmp_sq_pt']


def gen(ba):
    cal = mg.load_calibration_module(ba)
    rng = np.random.default_rng(1588)
    Nt, Nf = rc.NT, rc.NF
    freqs = torch.linspace(120e6, 180e6, Nf)
    times = torch.as_tensor(2459861.0 + np.arange(Nt) * 10.0 / 1440)
    arr = mg.hex_array(ba, 2, freqs)
    hex_ants, hex_vecs = list(arr.ants), np.asarray(arr.antvecs)
    ants = hex_ants + [max(hex_ants) + 4]
    vecs = np.concatenate([hex_vecs, [[60.0, -25.0, 0.5]]])
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    ants, vecs = [int(ants[k]) for k in order], vecs[order]
    assert ants != sorted(ants)
    antpos = {a: torch.as_tensor(v) for a, v in zip(ants, vecs)}
    bls_out, bls_red = rc.array_bls(ants, vecs)
    Nout, Nred = len(bls_out), len(bls_red)

    def cx(*shape):
        return torch.as_tensor(rng.normal(size=shape) + 1j * rng.normal(size=shape))

    out = dict(freqs=freqs, times=times, ants=np.array(ants), antvecs=vecs, bls_out=np.array(bls_out), bls_red=np.array(bls_red),
               data_red=cx(1, 1, Nred, Nt, Nf), data_phys=cx(1, 1, Nout, Nt, Nf),
               w=torch.as_tensor(rng.uniform(0.5, 2.0, size=(1, 1, Nout, Nt, Nf))))
    arows = {}

    terms, idx = cal.gen_coupling_terms(antpos, ants=[ants[1], ants[4]], min_len=1.0, max_EW=40.0, max_NS=20.0)
    out['terms_ants'] = np.array(terms)
    terms, idx = cal.gen_coupling_terms(antpos, compress_to_red=True, max_len=31.0)     # longer vectors: zeros
    cvecs = torch.stack([antpos[b] - antpos[a] for a, b in terms])
    infl = cal.CouplingInflate(-cvecs, antpos)
    out.update(inflate_vecs=-cvecs, inflate_idx=infl.idx, inflate_zeros=infl.zeros)

    for tag, kw in rc.GOLDEN_CASES.items():
        terms, idx = cal.gen_coupling_terms(antpos, compress_to_red=kw['compress'], no_auto_coupling=kw.get('no_auto', False),
                                            max_len=kw.get('term_max_len'))
        bls_in = bls_red if kw['use_reds'] else bls_out
        p = 0.3 * torch.as_tensor(rng.normal(size=(1, 1, len(terms), 1 if kw['tb'] else Nt, Nf, 2)))
        R = cal.VisModelResponse(param_type='com', times=None if kw['tb'] else times)
        m = cal.RedVisCoupling(p.clone(), freqs, antpos, terms, list(bls_in), list(bls_out), coupling_idx=idx, R=R,
                               p0=torch.zeros_like(p))
        setup = dict(use_reds=kw['use_reds'], copydata=True, include_second_order=kw['second'], **kw.get('setup', {}))
        m.setup_coupling(**setup)
        out['dly0_' + tag] = m.dly.clone()
        if 'min_dly' in kw:
            m.setup_coupling(min_dly=kw['min_dly'], **setup)
        for k in rc.TUPLES:
            for n, x in enumerate(getattr(m, k)):
                out['%s_%d_%s' % (k, n, tag)] = np.asarray(x, dtype=np.int64)
        for k in rc.TUPLES[:4]:
            t = getattr(m, k)
            assert len(set(zip(t[0].tolist(), t[1].tolist()))) == len(t[0]), (tag, k)
        if kw['use_reds']:
            out['red_bl_inds_' + tag] = np.array(m.red_bl_inds)
        hits = m.get_coupling_hits()
        keys = list(idx.keys())
        out.update({'terms_' + tag: np.array(terms), 'idx_keys_' + tag: np.array(keys),
                    'idx_vals_' + tag: np.array([idx[k] for k in keys]), 'dly_' + tag: m.dly.clone(), 'p_' + tag: p,
                    'hits_' + tag: np.array([hits[t] for t in terms])})
        if tag in AROWS_RECORDED:
            A = cal.configure_coupling_matrix_singlepath(
                antpos, bls_out, bl2red=None if not kw['use_reds'] else _bl2red(ba, antpos, bls_out, bls_in),
                include_second_order=kw['second'], **kw.get('setup', {}))
            arows[tag] = {'%d_%d' % bl: {'%d_%d' % k: v for k, v in row.items()} for bl, row in A.items()}
        vd = ba.dataset.VisData()
        vd.setup_meta(None, antpos)
        d = (out['data_red'] if kw['use_reds'] else out['data_phys']).clone().requires_grad_(True)
        vd.setup_data(bls_in, times, freqs, pol='ee', data=d)
        vout = m(vd)
        ((vout.data.real ** 2 + vout.data.imag ** 2) * out['w']).sum().backward()
        gd = d.grad.clone()
        if not kw['use_reds']:
            gd = gd + 2 * out['w'] * vout.data.detach()
        out.update({'V_' + tag: vout.data.detach(), 'gp_' + tag: m.params.grad.clone(), 'gd_' + tag: gd})
    arows['no_auto'] = {'%d_%d' % bl: {'%d_%d' % k: v for k, v in row.items()} for bl, row in
                        cal.configure_coupling_matrix_singlepath(antpos, bls_out[8:14], no_auto_coupling=True, min_len=1.0,
                                                                 max_EW=30.0, second_max_NS=16.0).items()}
    mg.save('redcoupling', **out)
    with open(os.path.join(HERE, 'redcoupling_arows.json'), 'w') as f:
        json.dump(arows, f, separators=(',', ':'))
    print('wrote redcoupling_arows.json %.1f kB' % (os.path.getsize(os.path.join(HERE, 'redcoupling_arows.json')) / 1e3))


def _bl2red(ba, antpos, bls_out, bls_in):
    reds, _, idx, _, _, _, _ = ba.telescope_model.build_reds(antpos, bls=bls_out, red_bls=bls_in, redtol=1.0)
    bl2red = {}
    for k in idx:
        bl2red[k] = reds[idx[k]][0]
        bl2red[k[::-1]] = reds[idx[k]][0][::-1]
    return bl2red


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen(mg.bootstrap_reference())
