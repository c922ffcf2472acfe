#!/usr/bin/env python3
"""
Golden vectors of the Fourier layer (reference fft.py and the averaging of dataset.py): every named window of gen_window
with and without edgecut, FFT.forward on a small complex tensor under the flag combinations of fft_common.FWD_CASES,
PeakDelay on tones between bins (plain, with abs, with a window and without the shift), average_data with weights, a
covariance and a truncated slot, VisData.bl_average on a hex-7 array (its own redundant groups, and explicit groups that
leave baselines out, with flags and inverse variances) and vis_wedge on the same array.  TEST INFRASTRUCTURE ONLY, like
make_golden.py, whose bootstrap it reuses; writes tests/golden/fft.npz, arrays only, everything float64 / complex128.

Finding (reference): average_data(truncate=True) indexes with a LIST of slices (dataset.py:4044-4050), which torch warns
about and will read as fancy indexing from 2.9 on; the restatement indexes with a tuple.
Finding (reference): PeakDelay without N fails on `None * tensor` (fft.py:173); every fixture passes N.

Usage:  python tests/golden/make_golden_fft.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import fft_common as fc   # noqa: E402


def hex7_vis(ba, rng, Nt=2, Nf=12):
    ants, vecs = ba.utils._make_hex(2, D=14.6)
    antpos = ba.utils.AntposDict(list(ants), np.asarray(vecs))
    bls = [(int(a), int(b)) for i, a in enumerate(ants) for b in ants[i + 1:]]
    data = torch.as_tensor(rng.normal(size=(1, 1, len(bls), Nt, Nf)) + 1j * rng.normal(size=(1, 1, len(bls), Nt, Nf)))
    times = np.array([2459861.0, 2459861.1])[:Nt]
    freqs = np.linspace(120e6, 131e6, Nf)
    return antpos, bls, data, times, freqs


def make_vd(ba, antpos, bls, data, times, freqs, **kw):
    vd = ba.dataset.VisData()
    vd.setup_meta(antpos=antpos)
    vd.setup_data(bls, times, freqs, pol='ee', data=data.clone(), **kw)
    return vd


def gen_fft(ba):
    ft, ds = ba.fft, ba.dataset
    rng = np.random.default_rng(83)
    cn = lambda *s: torch.as_tensor(rng.normal(size=s) + 1j * rng.normal(size=s))
    out = {}

    # windows
    for name in fc.WINDOWS:
        for N in (16, 9):
            out['win_%s_%d' % (name, N)] = ft.gen_window(name, N, **fc.WINDOW_KW.get(name, {}))
        out['win_%s_ec' % name] = ft.gen_window(name, 16, edgecut=(2, 3), **fc.WINDOW_KW.get(name, {}))

    # FFT.forward
    x = cn(2, 3, 12)
    out['fwd_x'] = x
    for i, (kw, dim) in enumerate(fc.FWD_CASES):
        xi = x if dim in (-1, 2) else x.movedim(-1, dim).contiguous()
        out['fwd_%d' % i] = ft.FFT(dim=dim, N=12, ndim=3, dx=0.5, **kw)(xi)
    wfull = torch.as_tensor(rng.uniform(0.2, 1.0, (2, 3, 12)))
    out.update(fwd_winfull=wfull, fwd_winfull_out=ft.FFT(dim=2, N=12)(x, win=wfull))

    # PeakDelay: 32 samples, tones between bins plus 1 % noise
    N = 32
    tones = np.array([3.3, 9.71, 16.48, 25.12, 30.9, 0.25])
    xp = torch.as_tensor(np.exp(2j * np.pi * tones[:, None] * np.arange(N) / N)) + 0.01 * cn(len(tones), N)
    xp = xp.reshape(2, 3, N)
    out.update(peak_x=xp, peak_tones=tones)
    for i, kw in enumerate(fc.PEAK_CASES):
        out['peak_%d' % i] = ft.PeakDelay(dim=2, N=N, ndim=3, dx=0.25, **kw)(xp)

    # average_data
    d = cn(2, 6, 4)
    index = torch.as_tensor([0, 1, 0, 2, 1, 2])
    w = torch.as_tensor(rng.uniform(0.5, 2.0, (2, 6, 4)))
    cov = torch.as_tensor(rng.uniform(0.5, 2.0, (2, 6, 4)))
    out.update(avg_x=d, avg_index=index, avg_w=w, avg_cov=cov)
    a, sw, ac = ds.average_data(d, 1, index, 3)
    out.update(avg0_data=a, avg0_wgts=sw)
    a, sw, ac = ds.average_data(d, -2, index, 3, wgts=w, cov=cov)
    out.update(avg1_data=a, avg1_wgts=sw, avg1_cov=ac)
    w1 = torch.as_tensor(rng.uniform(0.5, 2.0, (1, 6, 1)))
    a, sw, ac = ds.average_data(d, 1, index, 3, wgts=w1)
    out.update(avg2_w=w1, avg2_data=a, avg2_wgts=sw)
    # truncate: slot 2 collects what no output needs
    a, sw, ac = ds.average_data(d, -2, index, 3, wgts=w, cov=cov, truncate=True)
    out.update(avg3_data=a, avg3_wgts=sw, avg3_cov=ac)

    # bl_average on hex-7
    antpos, bls, data, times, freqs = hex7_vis(ba, rng)
    out.update(hex_antvecs=np.asarray(antpos.antvecs), hex_ants=np.asarray(antpos.ants), hex_bls=np.asarray(bls), hex_data=data,
               hex_times=times, hex_freqs=freqs)
    vd = make_vd(ba, antpos, bls, data, times, freqs)
    av = vd.bl_average()
    out.update(blavg_data=av.data, blavg_bls=np.asarray(av.bls))
    flags = torch.as_tensor(rng.uniform(size=data.shape) < 0.3)
    icov = torch.as_tensor(rng.uniform(0.5, 2.0, data.shape))
    out.update(hex_flags=flags, hex_icov=icov)
    reds = [[(0, 1), (1, 2), (3, 4)], [(0, 3), (1, 4)], [(2, 6)]]
    out['blavg_reds'] = np.asarray([(i, a, b) for i, red in enumerate(reds) for a, b in red])
    vd = make_vd(ba, antpos, bls, data, times, freqs, flags=flags.clone(), icov=icov.clone())
    av = vd.bl_average(reds=reds)
    out.update(blavg2_data=av.data, blavg2_flags=av.flags, blavg2_icov=av.icov, blavg2_bls=np.asarray(av.bls))

    # vis_wedge
    vd = make_vd(ba, antpos, bls, data, times, freqs)
    wv, FT = ft.vis_wedge(vd, window='bh', abs=True)
    out.update(wedge_data=wv.data, wedge_bls=np.asarray(wv.bls), wedge_delays=FT.freqs, wedge_win=FT.win.reshape(-1))
    mg.save('fft', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    ba = mg.bootstrap_reference()
    gen_fft(ba)
