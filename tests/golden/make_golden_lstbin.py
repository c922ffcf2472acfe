#!/usr/bin/env python3
"""
Golden vectors of the LST alignment stage (reference telescope_model.vis_rephase, dataset.VisData.lst_rephase /
time_nn_interp / time_average, dataset.average_data), on the case tables of lstbin_common:
 (a) vis_rephase: the phasor of every REPHASE_CASES entry, and its delay tau, formed from the reference's own rotation
     matrices (_eq2top_m, _top2eq_m) the way vis_rephase forms it (the function returns the phasor only);
 (b) VisData.lst_rephase(dLST=...) for a scalar and a per-time dLST;
 (c) VisData.time_nn_interp with and without rephasing, one case across the 2 pi wrap.  The reference's JD2LST needs astropy,
     which is stubbed here, so telescope_model.JD2LST is replaced by lstbin_common.jd2lst (a linear LST) for these records;
     the tests replace the product's JD2LST by the same function;
 (d) VisData.time_average(rephase=False) as the reference runs it (with flags set AND times dropped it raises -- its flag
     tensor is sized after the truncation --, so that combination is recorded under (e) only);
 (e) time_average(rephase=True) CANNOT run under the astropy stub (it needs astropy.units.sday), so for these cases the
     composition it performs is recorded: dLST = (mean time of the bin - time) 2 pi / sidereal day with the sidereal day of
     lstbin_common, the reference's vis_rephase, the product with the data, the reference's average_data with the index the
     method builds, and its flag / cov / icov rules.
Inputs are recorded next to the outputs.  TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes
tests/golden/lstbin.npz, arrays only, float64 / complex128.

Usage:  python tests/golden/make_golden_lstbin.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg      # noqa: E402
import lstbin_common as lc    # noqa: E402


def blvecs():
    v = np.asarray(lc.FIX_ANTVECS)
    return np.stack([v[lc.FIX_ANTS.index(j)] - v[lc.FIX_ANTS.index(i)] for i, j in lc.FIX_BLS])


def make_vd(ref, pol, times, data, icov, cov, flags):
    vd = ref.dataset.VisData()
    antpos = ref.utils.AntposDict(lc.FIX_ANTS, torch.as_tensor(np.asarray(lc.FIX_ANTVECS)))
    vd.setup_meta(telescope=types.SimpleNamespace(location=(lc.FIX_LON, lc.FIX_LAT)), antpos=antpos)
    T = lambda x: None if x is None else torch.as_tensor(x).clone()
    vd.setup_data(lc.FIX_BLS, torch.as_tensor(times), torch.as_tensor(lc.FIX_FREQS), pol=pol, data=T(data), flags=T(flags),
                  cov=T(cov), cov_axis=None, icov=T(icov))
    return vd


def record(out, name, vd):
    out[name + '_out_data'] = mg.npy(vd.data)
    out[name + '_out_times'] = mg.npy(vd.times)
    for k in ('flags', 'cov', 'icov'):
        v = getattr(vd, k)
        if v is not None:
            out[name + '_out_' + k] = mg.npy(v)


def main():
    ref = mg.bootstrap_reference()
    tm, ds = ref.telescope_model, ref.dataset
    torch.set_default_dtype(torch.float64)
    out = {}
    bv = blvecs()
    freqs = torch.as_tensor(lc.FIX_FREQS)

    # (a)
    for name, (dlst, lat) in lc.REPHASE_CASES.items():
        out['rephase_%s_phasor' % name] = mg.npy(tm.vis_rephase(torch.as_tensor(dlst), lat, torch.as_tensor(bv), freqs))
        d = torch.atleast_1d(torch.as_tensor(dlst))
        la = torch.atleast_1d(torch.as_tensor(lat)) * np.pi / 180
        rot = mg.npy(tm._eq2top_m(-d, la)) @ mg.npy(tm._top2eq_m(torch.tensor([0.0]), la))
        sdiff = rot[:, :, 2] - np.array([0.0, 0.0, 1.0])
        out['rephase_%s_tau' % name] = bv @ (sdiff / 2.99792458e8).T
    out['blvecs'] = bv

    # (b)
    for name, (pol, dlst) in lc.LSTR_CASES.items():
        data, icov, cov, flags = lc.fix_inputs('lstr_' + name, pol)
        vd = make_vd(ref, pol, lc.fix_times(lc.FIX_JD0), data, None, None, None)
        vd.lst_rephase(dLST=torch.as_tensor(dlst), inplace=True)
        out['lstr_%s_data' % name] = data
        record(out, 'lstr_' + name, vd)

    # (c)
    tm.JD2LST = lambda jd, lon: np.deg2rad(lc.jd2lst(np.asarray(jd), lon))
    for name, (pol, jd0, offs, rephase) in lc.NN_CASES.items():
        data, icov, cov, flags = lc.fix_inputs(name, pol)
        times = lc.fix_times(jd0)
        lsts = (np.deg2rad(lc.jd2lst(times[0], lc.FIX_LON)) + offs) % (2 * np.pi)
        vd = make_vd(ref, pol, times, data, icov, cov, flags)
        vd.time_nn_interp(lsts.copy(), rephase=rephase, inplace=True)
        for k, v in (('data', data), ('icov', icov), ('cov', cov), ('flags', flags), ('times', times), ('lsts', lsts)):
            out['%s_%s' % (name, k)] = v
        record(out, name, vd)
        if name == 'nn_wrap':
            assert lsts[-1] < lsts[0], 'the targets of nn_wrap must cross 2 pi'
            sl = lc.jd2lst(times, lc.FIX_LON)
            assert sl[-1] < sl[0], 'the data of nn_wrap must cross 2 pi'

    # (d), (e)
    for name, (pol, time_inds, use_icov, use_cov, use_flags, rephase) in lc.AVG_CASES.items():
        data, icov, cov, flags = lc.fix_inputs('avg_' + name, pol)
        icov, cov, flags = (icov if use_icov else None), (cov if use_cov else None), (flags if use_flags else None)
        times = lc.fix_times(lc.FIX_JD0)
        for k, v in (('data', data), ('icov', icov), ('cov', cov), ('flags', flags), ('times', times)):
            if v is not None:
                out['avg_%s_%s' % (name, k)] = v
        vd = make_vd(ref, pol, times, data, icov, cov, flags)
        tinds = None if time_inds is None else [torch.as_tensor(t) for t in time_inds]
        if not rephase:
            vd.time_average(time_inds=tinds, rephase=False, inplace=True)
            record(out, 'avg_' + name, vd)
            continue
        # the composition time_average(rephase=True) performs (see the module docstring)
        Nt, Nmax = len(times), len(time_inds)
        index = torch.ones(Nt, dtype=torch.int64) * Nmax
        for i, t in enumerate(time_inds):
            index[torch.as_tensor(t)] = i
        Nout = index.unique().numel()
        truncate = bool(Nmax in index)
        tt = torch.as_tensor(times)
        avg_times = torch.zeros(Nout).index_add_(0, index, tt) / torch.zeros(Nout).index_add_(0, index, torch.ones_like(tt))
        dLST = (avg_times[index] - tt) * 2 * np.pi / (lc.SDAY_SEC / 86400.0)
        phs = tm.vis_rephase(dLST, lc.FIX_LAT, torch.as_tensor(bv), freqs)
        wg = vd.icov
        cv = vd.cov if vd.cov is not None else (1 / vd.icov.clip(1e-60) if vd.icov is not None else None)
        avg_data, sum_w, avg_cov = ds.average_data(vd.data * phs, -2, index, Nout, wgts=wg, cov=cv, truncate=truncate)
        out['avg_%s_out_data' % name] = mg.npy(avg_data)
        out['avg_%s_out_times' % name] = mg.npy(avg_times[:-1] if truncate else avg_times)
        if vd.flags is not None:
            cnt = torch.zeros(avg_data.shape[:-2] + (Nout, avg_data.shape[-1]), dtype=torch.int64)
            cnt.index_add_(-2, index, (~vd.flags).to(torch.int64))
            fl = cnt == 0                                   # flagged where every member is: what ~(index_add_ of ~flags) states
            out['avg_%s_out_flags' % name] = mg.npy(fl[..., :-1, :] if truncate else fl)
        if vd.icov is not None:
            out['avg_%s_out_icov' % name] = mg.npy(1 / avg_cov.clip(1e-60))
        if vd.cov is not None:
            out['avg_%s_out_cov' % name] = mg.npy(avg_cov)

    mg.save('lstbin', **out)


if __name__ == '__main__':
    main()
