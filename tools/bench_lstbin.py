#!/usr/bin/env python3
"""
LST binning at the HERA-128 shape: 8128 baselines, 60 integrations into 6 bins of 10, 256 channels, complex64, 1 pol, with
inverse-variance weights, variances and flags.  The fused path (VisData.time_average(rephase=True): ONE launch of
rime_vis_timeavg_fwd, the phasor generated in registers) against the reference's chain written with torch ops on the same
GPU: the phasor tensor (phase in float64, reduced, exponentiated in complex64 -- cheaper than the reference's complex128),
the product with the data, dataset.average_data (three index_add_ passes and two divisions) and the flag count.  The torch
chain is the baseline, not the code under test.  Both run in this process, alternating, after a warm-up; every repetition is
timed with device events.  Reported: median and spread of each, their ratio, the bytes per second of the fused launch against
its algorithmic traffic (one read of data, weights, cov and flags, one write of the bins) as a fraction of a copy_ of the same
number of bytes in this process and of the 8 TB/s HBM3E peak, and whether two runs of each path gave the same bits.

  python tools/bench_lstbin.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import dataset, ops, telescope_model, utils  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    ts = np.asarray(ts)
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return med, q3 - q1, ts.min(), ts.max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_lstbin.py measures on the GPU; none found')
    assert a.reps >= 20
    dev = 'cuda:0'
    Nt, Nbin, Nf = 60, 6, 256
    ants, vecs = utils._make_hex(7, D=14.6)
    ants, vecs = list(ants) + [len(ants)], np.vstack([vecs, [[383.7, -211.3, 0.0]]])
    bls = [(p, q) for i, p in enumerate(ants) for q in ants[i + 1:]]
    Nbl = len(bls)
    g = torch.Generator(device=dev).manual_seed(5)
    shape = (1, 1, Nbl, Nt, Nf)
    data = torch.complex(torch.randn(shape, generator=g, device=dev), torch.randn(shape, generator=g, device=dev))
    icov = torch.rand(shape, generator=g, device=dev) + 0.5
    cov = 1 / icov
    flags = torch.rand(shape, generator=g, device=dev) < 0.1
    freqs = torch.linspace(100e6, 200e6, Nf, device=dev, dtype=torch.float64)
    times = 2459861.3 + np.arange(Nt) * 10.0 / 86400
    time_inds = [list(range(10 * k, 10 * k + 10)) for k in range(Nbin)]
    vd = dataset.VisData()
    vd.setup_meta(telescope=telescope_model.TelescopeModel((21.42827, -30.72148)), antpos=utils.AntposDict(ants, vecs))

    def fresh():
        vd.setup_data(bls, times, freqs, pol='ee', data=data, flags=flags)
        vd.cov, vd.icov, vd.cov_axis = cov, icov, None       # no clone, no log-determinant pass: the average alone is timed
        return vd

    # what time_average hands the kernel, for the torch chain
    index = torch.as_tensor(np.repeat(np.arange(Nbin), 10), device=dev)
    avg_times = times.reshape(Nbin, 10).mean(1)
    dlst = (np.repeat(avg_times, 10) - times) * 2 * np.pi / (dataset.SDAY_SEC / 86400.0)
    tau = fresh()._rephase_tau(dlst).to(dev)

    def fused():
        out = fresh().time_average(time_inds=time_inds, rephase=True, inplace=False)
        return out.data, out.cov, out.flags

    plan = ops.TimeAvgPlan(time_inds, Nt)

    def fused_launch():
        return ops.vis_timeavg(data, plan, wgts=icov, cov=cov, flags=flags, tau=tau, freqs=freqs)

    def chain():
        ph = freqs * tau[..., None]
        phs = torch.exp(2j * np.pi * (ph - torch.round(ph)).to(torch.float32))
        avg, sw, acov = dataset.average_data(data * phs, -2, index, Nbin, wgts=icov, cov=cov)
        count = torch.zeros(avg.shape, dtype=torch.int64, device=dev)
        count.index_add_(-2, index, (~flags).to(torch.int64))
        return avg, acov, count == 0

    with torch.no_grad():
        yf, yc = fused(), chain()
        err = ((yf[0] - yc[0]).abs().max() / yc[0].abs().max()).item()
        assert err < 1e-5 and torch.equal(yf[2], yc[2]), err
        assert ((yf[1] - yc[1]).abs().max() / yc[1].abs().max()).item() < 1e-5
        same = {}
        for k, fn in (('fused', fused), ('torch', chain)):
            p, q = fn(), fn()
            same[k] = all(torch.equal(torch.view_as_real(x) if x.is_complex() else x, torch.view_as_real(y) if y.is_complex() else y)
                          for x, y in zip(p, q))
        n = data.numel()
        nbytes = n * (8 + 4 + 4 + 1) + (n // 10) * (8 + 4 + 4 + 1)       # data, weights, cov, flags read; avg, sum_w, avg_cov, flags written
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        runs = {'fused time_average': fused, 'fused launch alone': fused_launch, 'torch chain': chain,
                'copy (same bytes)': lambda: dst.copy_(src)}
        t = {k: [] for k in runs}
        for _ in range(a.warmup):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):                                          # alternating, so that drift hits all alike
            for k, fn in runs.items():
                t[k].append(timed(fn))
    s = {k: stats(v) for k, v in t.items()}
    lines = ['LST binning, fused HIP path vs phasor + multiply + average_data in torch; %d baselines, %d integrations into %d bins, '
             '%d channels, complex64; %d reps after %d warm-up [ms]   (fused vs torch data: %.1e)' % (Nbl, Nt, Nbin, Nf, a.reps, a.warmup, err)]
    for k in runs:
        lines.append('  %-19s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((k,) + s[k]))
    bw, cbw = nbytes / s['fused launch alone'][0] / 1e9, nbytes / s['copy (same bytes)'][0] / 1e9
    lines.append('  fused launch: %.2f TB/s of its algorithmic traffic (%.1f MB) = %.2f of the %.0f TB/s HBM peak; copy_ of the same '
                 'bytes (half read, half written): %.2f TB/s; fraction of the copy %.2f'
                 % (bw, nbytes / 1e6, bw * 1e12 / HBM_PEAK, HBM_PEAK / 1e12, cbw, bw / cbw))
    f, c = s['fused time_average'], s['torch chain']
    lines.append('  ratio torch / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused faster beyond the spread: %s'
                 % (c[0] / f[0], c[0] - f[0], max(f[1], c[1]), (c[0] - f[0]) > max(f[1], c[1])))
    lines.append('  bit-identical across two runs: fused %s, torch %s' % (same['fused'], same['torch']))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
