#!/usr/bin/env python3
"""
The L-BFGS search direction at optimiser sizes: the fused path (bfgs.LBFGS.hvp: one rime_lbfgs_dots launch, the read-back of
2 m float64, the m x m recurrence on the host, the upload of 2 m coefficients, one rime_lbfgs_combine launch) against the
two-loop recursion written with torch ops on the same tensors (4 m dependent vector operations, two of them reductions with
a read-back each -- the form of the reference's two_loop_recursion).  The torch loop is the baseline, not the code under
test.  Both run in this process, alternating, after a warm-up; a direction is timed with the host clock between device
synchronisations (either path ends in host work), the two kernels of the fused path on their own with device events.
Reported: median and spread of each, their ratio, and the bytes per second of the two passes against their algorithmic
traffic (dots: 2 m + 2 vectors read; combine: 2 m + 2 read, one written).

  history m = 10 and m = 100;  N = 786 432 (the C2 parameter count, 12 288 x 64) and N = 2^24 (a C4-like count whose
  100 pairs, 13.4 GB in float32, fit in memory);  float32, a diagonal starting matrix

  python tools/bench_lbfgs.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import bfgs  # noqa: E402


def torch_two_loop(vec, s, y, rho, H):
    """Nocedal & Wright, algorithm 7.4, one torch op per line"""
    q = vec
    m = len(s)
    alpha = [None] * m
    for i in reversed(range(m)):
        alpha[i] = rho[i] * (s[i] @ q)
        q = q - alpha[i] * y[i]
    r = H * q
    for i in range(m):
        beta = rho[i] * (y[i] @ r)
        r = r + s[i] * (alpha[i] - beta)
    return r


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_timed(fn):
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
        sys.exit('bench_lbfgs.py measures on the GPU; none found')
    dev = 'cuda:0'
    gen = torch.Generator(device=dev).manual_seed(23)
    rn = lambda n: torch.randn(n, generator=gen, device=dev, dtype=torch.float32)
    lines = ['L-BFGS direction, fused path vs the two-loop recursion in torch ops; float32, %d reps after %d warm-up [ms]' % (a.reps, a.warmup)]
    for N in (12288 * 64, 2 ** 24):
        for m in (10, 100):
            d = torch.rand(N, generator=gen, device=dev) + 0.5
            x = torch.zeros(N, device=dev, requires_grad=True)
            opt = bfgs.LBFGS((x,), H0=d, history_size=m, update_Hdiag=True)
            for _ in range(m):
                s = rn(N)
                opt.update_hessian(s, s * (torch.rand(N, generator=gen, device=dev) + 0.5))
            assert len(opt._s) == m
            v = rn(N)
            S, Y, rho, H = list(opt._s), list(opt._y), [torch.tensor(r, device=dev, dtype=torch.float32) for r in opt._rho], opt._Hdiag
            rf, rt = opt.hvp(v), torch_two_loop(v, S, Y, rho, H)
            err = ((rf - rt).abs().max() / rt.abs().max()).item()
            h = opt._hist
            ab = np.zeros(m)
            runs = {'fused direction': lambda: opt.hvp(v), 'torch two-loop': lambda: torch_two_loop(v, S, Y, rho, H)}
            kern = {'dots pass': lambda: _lib_dots(h, v), 'combine pass': lambda: h.combine(v, ab, ab, 1.0)}
            t = {k: [] for k in list(runs) + list(kern)}
            for _ in range(a.warmup):
                for fn in list(runs.values()) + list(kern.values()):
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.reps):                                      # alternating, so that drift hits all alike
                for k, fn in runs.items():
                    t[k].append(host_timed(fn))
                for k, fn in kern.items():
                    t[k].append(event_timed(fn))
            st = {k: stats(x_) for k, x_ in t.items()}
            lines.append(' N = %d, m = %d   (fused vs torch, two float32 evaluations: %.1e)' % (N, m, err))
            for k in t:
                lines.append('  %-16s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((k,) + st[k]))
            f, c = st['fused direction'], st['torch two-loop']
            lines.append('  ratio torch / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused faster beyond the spread: %s'
                         % (c[0] / f[0], c[0] - f[0], max(f[1], c[1]), (c[0] - f[0]) > max(f[1], c[1])))
            bd, bc = (2 * m + 2) * N * 4, (2 * m + 3) * N * 4
            lines.append('  dots pass %.2f TB/s of %.1f MB; combine pass %.2f TB/s of %.1f MB (the combine time includes the upload of '
                         'its 2 m coefficients)' % (bd / st['dots pass'][0] / 1e9, bd / 1e6, bc / st['combine pass'][0] / 1e9, bc / 1e6))
            del opt, S, Y, h, runs, kern
            torch.cuda.empty_cache()
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


def _lib_dots(h, v):
    """the dots launch without its read-back: the two kernels alone between the events"""
    from bayeslim_amd import _lib
    from bayeslim_amd.ops import _ptr, _stream
    S, Y, m = h._tables()
    if getattr(h, '_bench_out', None) is None or h._bench_out.shape[1] != m:
        h._bench_out = torch.empty((2, m), dtype=torch.float64, device=h.device)
    _lib.check(_lib.lib.rime_lbfgs_dots(h.code, S, Y, m, h.N, _ptr(v), _ptr(h.d), -1, _ptr(h._bench_out), _ptr(h.ws),
                                        h.ws.numel() * 8, _stream()), 'rime_lbfgs_dots')


if __name__ == '__main__':
    main()
