#!/usr/bin/env python3
"""
LinearModel at the shapes the models use it: the fused HIP path (linear_model.LinearModel -> ops.lm_apply, one launch forward
and one backward, plus a torch index_add_ when a gather is scattered back) against the reference's own expression chain
written with torch ops on the same GPU (params * coeff, index_select, A @ params / params @ A.T, .real:
linear_model.py:121-169).  The chain is the baseline, not the code under test.  Both run in this process, alternating, after
a warm-up; every repetition is timed with device events; forward alone (no gradient) and forward plus backward (of the sum
of the output).  Reported: the median and spread of each, their ratio, and the bytes per second of the fused forward
against its algorithmic traffic (input read once, output written once), as a fraction of what a copy_ of the same number of
bytes reaches in this process.

  (a) sky    (1, 1, 8, 196608)  -> 256 along -2, float32
  (b) the same with complex Fourier coefficients (1, 1, 16, 196608) and out_real
  (c) beam   (1, 1, 1, 8, 32760) -> 256 along -2
  (d) gains  (1, 1, 128, 8, 6) complex -> 256 along -1
  (e) (a) with a coeff vector and an idx
  (f) a middle axis in front of a short one: (1, 128, 8, 6) -> 256 along -2 (I = 6), the strided mapping at small I

  python tools/bench_lm.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import linear_model as lm  # noqa: E402

NF = 256


def chain(A, dim, coeff=None, idx=None, out_real=False):
    """the reference's LinearModel.forward for dim = -2 / -1 (linear_model.py:121-169)"""
    def run(p):
        if coeff is not None:
            p = p * coeff
        if idx is not None:
            p = torch.index_select(p, dim, idx)
        out = A @ p if dim == -2 else p @ A.T
        return out.real if out_real else out
    return run


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


def fwd_bwd(fn, x):
    def run():
        xg = x.detach().requires_grad_(True)
        y = fn(xg)
        (y.real if y.is_complex() else y).sum().backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_lm.py measures on the GPU; none found')
    assert a.reps >= 20
    dev = 'cuda:0'
    rng = np.random.default_rng(17)
    rn = lambda *s: torch.as_tensor(rng.normal(size=s), dtype=torch.float32, device=dev)
    cn = lambda *s: torch.complex(rn(*s), rn(*s))
    freqs = torch.linspace(120e6, 180e6, NF, dtype=torch.float64)
    poly = lambda n: lm.gen_poly_A(freqs, n, basis='legendre').to(torch.float32).to(dev)
    four = lm.gen_fourier_A(freqs, Ndeg=16)[0].to(torch.complex64).to(dev)
    idx = torch.as_tensor([9, 0, 1, 2, 2, 4, 6, 7], device=dev)
    cases = [
        ('(a) sky (1,1,8,196608) -> 256, dim -2, f32', rn(1, 1, 8, 196608), poly(8), -2, {}),
        ('(b) sky, complex Fourier (1,1,16,196608) -> 256, out_real', cn(1, 1, 16, 196608), four, -2, dict(out_real=True)),
        ('(c) beam (1,1,1,8,32760) -> 256, dim -2, f32', rn(1, 1, 1, 8, 32760), poly(8), -2, {}),
        ('(d) gains (1,1,128,8,6) complex -> 256, dim -1', cn(1, 1, 128, 8, 6), poly(6).to(torch.complex64), -1, {}),
        ('(e) sky (1,1,10,196608) -> 256 with coeff vector and idx (8 of 10)', rn(1, 1, 10, 196608), poly(8), -2,
         dict(coeff=torch.as_tensor(rng.uniform(0.5, 2, (1, 1, 10, 1)), dtype=torch.float32, device=dev), idx=idx)),
        ('(f) small inner axis (1,128,8,6) -> 256, dim -2 (I = 6)', rn(1, 128, 8, 6), poly(8), -2, {}),
    ]
    lines = ['LinearModel forward, fused HIP path vs the reference chain in torch; %d reps after %d warm-up [ms]' % (a.reps, a.warmup)]
    for name, x, A, dim, kw in cases:
        L = lm.LinearModel('custom', A=A, dim=dim, **kw)
        ref = chain(A, dim, **kw)
        with torch.no_grad():
            yf, yr = L(x), ref(x)
        err = ((yf - yr).abs().max() / yr.abs().max()).item()
        assert yf.shape == yr.shape and err < 1e-4, (name, err)         # two float32 evaluations of the same product
        nbytes = x.numel() * x.element_size() + yf.numel() * yf.element_size()
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        runs = {'fused fwd': lambda: L(x), 'chain fwd': lambda: ref(x), 'copy': lambda: dst.copy_(src),
                'fused fwd+bwd': fwd_bwd(L, x), 'chain fwd+bwd': fwd_bwd(ref, x)}
        t = {k: [] for k in runs}
        for _ in range(a.warmup):
            for k, fn in runs.items():
                with torch.set_grad_enabled('bwd' in k):
                    fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):                                         # alternating, so that drift hits all alike
            for k, fn in runs.items():
                with torch.set_grad_enabled('bwd' in k):
                    t[k].append(timed(fn))
        s = {k: stats(v) for k, v in t.items()}
        lines.append(' %s   (fused vs chain: %.1e)' % (name, err))
        for k in runs:
            lines.append('  %-14s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((k,) + s[k]))
        bw, cbw = nbytes / s['fused fwd'][0] / 1e9, nbytes / s['copy'][0] / 1e9
        lines.append('  fused fwd: %.2f TB/s of its algorithmic traffic (%.1f MB); copy_ of the same bytes (half read, half written): '
                     '%.2f TB/s; fraction %.2f' % (bw, nbytes / 1e6, cbw, bw / cbw))
        for tag in ('fwd', 'fwd+bwd'):
            f, c = s['fused ' + tag], s['chain ' + tag]
            lines.append('  %-7s ratio chain / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused faster beyond the spread: %s'
                         % (tag, c[0] / f[0], c[0] - f[0], max(f[1], c[1]), (c[0] - f[0]) > max(f[1], c[1])))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
