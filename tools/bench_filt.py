#!/usr/bin/env python3
"""
Forward + backward of a baseline-dependent frequency filter at the headline shape: visibilities (1, 1, 8128, 8, 256)
complex64, 16 residual filters of 256 x 256 assigned by baseline length.  The fused HIP path (filt.WedgeFilter -> ops.filt_apply,
one launch per direction) against the reference's formulation written with torch ops on the GPU (a Python loop over the groups:
gather the group's baselines, complex einsum with its G, scatter back; autograd walks the same chain in reverse).  The loop is
the baseline, not the code under test.  Both run in this process, alternating, after a warm-up; every repetition is timed with
device events; reported are the median and the spread of each, their ratio, and the kernel launches of one step of each as
torch.profiler counts them.

  python tools/bench_filt.py [--reps 20] [--warmup 3] [--real] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import filt  # noqa: E402

NBL, NT, NF, NFILT = 8128, 8, 256, 16


def make(dev, cplx):
    rng = np.random.default_rng(11)
    f = torch.linspace(0.0, 1.0, NF, dtype=torch.float64)
    blen = np.sort(rng.uniform(14.0, 300.0, NBL))[rng.permutation(NBL)]          # groups interleaved along the baseline axis
    grp = np.minimum((blen - 14.0) / (300.0 - 14.0) * NFILT, NFILT - 1).astype(int)
    bls = [(0, i + 1) for i in range(NBL)]
    members = []
    for i in range(NFILT):
        C = filt.sinc_cov(f, 1.0 / (4.0 + 2.0 * i))
        if cplx:
            C = C * filt.phasor_mat(f, 1.0 + i)
        members.append(filt.GPFilter(C, torch.eye(NF, dtype=torch.float64) * 1e-3, residual=True, inv='inv'))
    f2b = {i: [bl for bl, k in zip(bls, grp) if k == i] for i in range(NFILT)}
    wedge = filt.WedgeFilter(members, f2b, bls=bls)
    wedge.push(torch.device(dev))
    wedge.push(torch.float32)
    x = torch.as_tensor(rng.normal(size=(1, 1, NBL, NT, NF)) + 1j * rng.normal(size=(1, 1, NBL, NT, NF)),
                        dtype=torch.complex64, device=dev).requires_grad_(True)
    w = torch.as_tensor(rng.normal(size=(1, 1, NBL, NT, NF)) + 1j * rng.normal(size=(1, 1, NBL, NT, NF)),
                        dtype=torch.complex64, device=dev)
    Gs = [m.G.to(torch.complex64) for m in members]
    idx = [torch.as_tensor(np.nonzero(grp == i)[0], device=dev) for i in range(NFILT)]

    def loop(v):
        out = v.clone()
        for G, ix in zip(Gs, idx):
            sub = out[..., ix, :, :]
            out[..., ix, :, :] = sub - torch.einsum('ij,abcdj->abcdi', G, sub)
        return out

    return wedge, loop, x, w


def step(fn, x, w):
    x.grad = None
    out = fn(x)
    out.backward(w)
    return out


def timed(fn, x, w):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step(fn, x, w)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def launches(fn, x, w):
    """device kernels of one forward + backward step, or None when the profiler reports none"""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(fn, x, w)
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]
        kern = [e for e in evs if 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower()]
        return (len(kern), sum('filt_kernel' in e.name for e in kern)) if evs else None
    except Exception:
        return None


def stats(ts):
    ts = np.asarray(ts)
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return med, q3 - q1, ts.min(), ts.max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--real', action='store_true', help='real filter matrices instead of complex ones')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_filt.py measures on the GPU; none found')
    assert a.reps >= 10
    dev = 'cuda:0'
    wedge, loop, x, w = make(dev, not a.real)
    of, gf = step(wedge, x, w).detach(), x.grad.clone()
    ol, gl = step(loop, x, w).detach(), x.grad.clone()
    eo = ((of - ol).abs().max() / x.detach().abs().max()).item()
    eg = ((gf - gl).abs().max() / w.abs().max()).item()
    assert eo < 1e-4 and eg < 1e-4, (eo, eg)                  # two float32 summation orders of the same products
    for _ in range(a.warmup):
        step(wedge, x, w)
        step(loop, x, w)
    torch.cuda.synchronize()
    t = {'fused': [], 'loop': []}
    for _ in range(a.reps):                                   # alternating, so that drift hits both alike
        t['fused'].append(timed(wedge, x, w))
        t['loop'].append(timed(loop, x, w))
    sf, sl = stats(t['fused']), stats(t['loop'])
    flop = 8 * NBL * NT * NF * NF * 2                         # 8 per complex multiply-add, forward + backward
    lines = ['wedge filter (1, 1, %d, %d, %d) complex64, %d %s filters %d x %d by baseline length, residual; %d reps after %d '
             'warm-up, fwd + bwd [ms]' % (NBL, NT, NF, NFILT, 'real' if a.real else 'complex', NF, NF, a.reps, a.warmup)]
    for tag, s in (('fused', sf), ('loop', sl)):
        lines.append('  %-6s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((tag,) + s))
    if not a.real:
        lines.append('  fused: %.1f TFLOP/s of real arithmetic at the median' % (flop / sf[0] / 1e9))
    margin = sl[0] - sf[0]
    lines.append('  ratio loop / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused vs loop: out %.1e grad %.1e' % (
        sl[0] / sf[0], margin, max(sf[1], sl[1]), eo, eg))
    lines.append('  fused below loop by more than the larger spread: %s' % (margin > max(sf[1], sl[1])))
    for tag, fn in (('fused', wedge), ('loop', loop)):
        n = launches(fn, x, w)
        lines.append('  %-6s kernel launches per step: %s' % (tag, 'not measured' if n is None else '%d (filt_kernel: %d)' % n))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
