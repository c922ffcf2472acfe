#!/usr/bin/env python3
"""
Forward + backward of the SFB radial transform: the fused HIP path (ops.sfb_radial, one launch per direction) against the
reference's formulation written with torch ops on the GPU (a Python loop over degrees: slice, reshape, matmul with the
complex-typed matrix, indexed assignment; autograd walks the same chain back).  The loop is the baseline, not the code under
test.  Both run in this process, alternating, after a warm-up; every repetition is timed with device events; reported are the
median and the spread (interquartile range, and min .. max) of each, and their ratio.

Shapes: `fixture` (tests/golden/sfb.npz: lmax 6, Nr 23, Nlmn 335, batch (2, 1)) and `c3` (gen_lm(128): 8385 columns, Nr 128,
Nk 64 per degree, random matrices -- timing needs no Bessel functions --, batch (1, 1), complex64).

  python tools/bench_sfb.py [--reps 30] [--warmup 5] [--out FILE]
  python tools/bench_sfb.py --only fused|loop --shape c3 --reps 10 --warmup 0      # for a kernel trace: launch counts
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import sph_harm  # noqa: E402


def make_shape(name, dev):
    rng = np.random.default_rng(3)
    if name == 'fixture':
        with np.load(os.path.join(ROOT, 'tests', 'golden', 'sfb.npz')) as f:
            l, nk, G = f['shell_l'], f['shell_nk'], f['shell_gln']
            keys = [int(k) for k in f['shell_keys']]
        mats = np.split(G, np.cumsum(nk)[:-1])
        batch = (2, 1)
    else:
        l, _ = sph_harm.gen_lm(128, real_field=True)
        keys = list(range(129))
        mats = [rng.normal(size=(64, 128)) / 8 for _ in keys]
        batch = (1, 1)
    gln = {k: torch.as_tensor(m, dtype=torch.float32) for k, m in zip(keys, mats)}
    kln = {k: np.arange(len(m), dtype=np.float64) for k, m in zip(keys, mats)}
    sfb = sph_harm.SFBModel()
    sfb.setup_gln(l, gln=gln, kln=kln)
    p = torch.as_tensor(rng.normal(size=batch + (sfb.Nlmn,)) + 1j * rng.normal(size=batch + (sfb.Nlmn,)),
                        dtype=torch.complex64, device=dev).requires_grad_(True)
    w = torch.as_tensor(rng.normal(size=batch + (sfb.Nr, sfb.Nlm)) + 1j * rng.normal(size=batch + (sfb.Nr, sfb.Nlm)),
                        dtype=torch.complex64, device=dev)
    # baseline operands: complex-typed transposed matrices on the device, index objects as the reference keeps them
    gT = {k: gln[k].to(dev).T.to(torch.complex64) for k in keys}
    idx = {k: (sfb.alm_idx[k] if isinstance(sfb.alm_idx[k], slice) else torch.as_tensor(sfb.alm_idx[k], device=dev)) for k in keys}

    def loop(params):
        out = torch.zeros(params.shape[:-1] + (sfb.Nr, sfb.Nlm), dtype=params.dtype, device=params.device)
        for k in keys:
            q = params[..., sfb.params_idx[k]].reshape(params.shape[:-1] + (-1, sfb.alm_shape[k][1]))
            out[..., idx[k]] = gT[k] @ q
        return out

    return sfb, loop, p, w


def step(fn, p, w):
    p.grad = None
    out = fn(p)
    out.backward(w)
    return out


def timed(fn, p, w):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step(fn, p, w)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    ts = np.asarray(ts)
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return med, q3 - q1, ts.min(), ts.max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--shape', default=None, choices=['fixture', 'c3'])
    ap.add_argument('--only', default=None, choices=['fused', 'loop'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_sfb.py measures on the GPU; none found')
    dev = torch.device('cuda', 0)
    lines = []
    for name in ([a.shape] if a.shape else ['fixture', 'c3']):
        sfb, loop, p, w = make_shape(name, dev)
        paths = {'fused': sfb, 'loop': loop}
        if a.only:
            for _ in range(max(a.warmup, 0) + a.reps):
                step(paths[a.only], p, w)
            torch.cuda.synchronize()
            lines.append('%s %s: %d forward + backward steps run (%d degrees)' % (name, a.only, a.warmup + a.reps, len(sfb.gln)))
            continue
        of, gf = step(sfb, p, w).detach(), p.grad.clone()
        ol, gl = step(loop, p, w).detach(), p.grad.clone()
        eo = ((of - ol).abs().max() / ol.abs().max()).item()
        eg = ((gf - gl).abs().max() / gl.abs().max()).item()
        assert eo < 1e-5 and eg < 1e-4, (eo, eg)            # two float32 summation orders of the same products
        for _ in range(a.warmup):
            step(sfb, p, w)
            step(loop, p, w)
        torch.cuda.synchronize()
        t = {'fused': [], 'loop': []}
        for _ in range(a.reps):                               # alternating, so that drift hits both alike
            t['fused'].append(timed(sfb, p, w))
            t['loop'].append(timed(loop, p, w))
        sf, sl = stats(t['fused']), stats(t['loop'])
        lines.append('%-8s Nlm %5d Nr %4d Nlmn %7d degrees %4d batch %s complex64, %d reps after %d warm-up, fwd + bwd [ms]' % (
            name, sfb.Nlm, sfb.Nr, sfb.Nlmn, len(sfb.gln), tuple(p.shape[:-1]), a.reps, a.warmup))
        for tag, s in (('fused', sf), ('loop', sl)):
            lines.append('  %-6s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((tag,) + s))
        margin = sl[0] - sf[0]
        lines.append('  ratio loop / fused %.1f   median difference %.4f ms   larger IQR %.4f ms   fused vs loop: out %.1e grad %.1e' % (
            sl[0] / sf[0], margin, max(sf[1], sl[1]), eo, eg))
        lines.append('  fused below loop by more than the larger spread: %s' % (margin > max(sf[1], sl[1])))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
