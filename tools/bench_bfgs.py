#!/usr/bin/env python3
"""
One dense BFGS iteration at optimiser sizes: the two passes of csrc/bfgs.hip (rime_bfgs_matvec for u = H g, rime_bfgs_rank2 for
the correction of H in place) against two baselines written with torch ops on the same tensors:

  (a) the reference's form  V = I - rho y s^T;  H = V^T H V + rho s s^T  (two N x N x N products, three N x N temporaries)
  (b) the O(N^2) restatement in torch ops: w = torch.mv(H, y) and three addr_ (-rho s w^T, -rho w s^T, b s s^T)

The baselines are not the code under test.  All three run in this process, alternating, after a warm-up, each timed with
device events around its launches (no host work in between); the two kernels also on their own.  Reported: median and spread
of each, the ratios, and the bytes per second of the kernel iteration against its algorithmic traffic 3 N^2 sizeof(T)
(H read once for the product, read and written once for the correction), per pass N^2 and 2 N^2.

  N = 1024 and 4096, float32 and float64

  python tools/bench_bfgs.py [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import bfgs  # noqa: E402


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


def reference_form(H, s, y, rho, eye):
    V = eye - rho * torch.outer(y, s)
    return V.T @ H @ V + rho * torch.outer(s, s)


def torch_rank2(H, s, y, rho, b=None):
    """mv and three addr_; b = rho^2 (y . H y) + rho is read back where it is not given (the timed loop gives it)"""
    w = torch.mv(H, y)
    b = rho * rho * float(y @ w) + rho if b is None else b
    return H.addr_(s, w, alpha=-rho).addr_(w, s, alpha=-rho).addr_(s, s, alpha=b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_bfgs.py measures on the GPU; none found')
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(29)
    lines = ['dense BFGS iteration, kernels vs torch baselines; %d reps after %d warm-up, device events [ms]' % (a.reps, a.warmup)]
    for dtype in (torch.float32, torch.float64):
        for N in (1024, 4096):
            rn = lambda *shape: torch.randn(*shape, generator=gen, device=dev, dtype=dtype)
            B = rn(N, N) / N ** 0.5
            H0 = B @ B.T + torch.eye(N, device=dev, dtype=dtype)
            H0 = 0.5 * (H0 + H0.T)
            s, g = rn(N), rn(N)
            y = torch.linalg.solve(H0, s) + 0.01 * rn(N)           # a pair with curvature: y . s > 0
            rho = 1.0 / float(y @ s)
            assert rho > 0
            dense = bfgs._Dense(N, dtype, dev)
            eye = torch.eye(N, device=dev, dtype=dtype)

            # the three forms compute the same matrix
            Hk = H0.clone()
            w = dense.matvec(Hk, y)
            dense.rank2(Hk, s, w, -rho, rho * rho * float(y @ w) + rho)
            Hr = reference_form(H0, s, y, rho, eye)
            Ht = torch_rank2(H0.clone(), s, y, rho)
            err = (float((Hk - Hr).abs().max() / Hr.abs().max()), float((Ht - Hr).abs().max() / Hr.abs().max()))

            Hw = H0.clone()                                        # updated in place over and over with a tiny correction
            small = 1e-6 * rho

            def kernels():
                u = dense.matvec(Hw, g)
                dense.rank2(Hw, s, u, -small, small)

            runs = {'kernels (matvec + rank2)': kernels,
                    '(a) V^T H V + outer': lambda: reference_form(H0, s, y, rho, eye),
                    '(b) mv + 3 addr_': lambda: torch_rank2(Hw, s, y, small, small),
                    'matvec pass': lambda: dense.matvec(Hw, g),
                    'rank2 pass': lambda: dense.rank2(Hw, s, y, -small, small)}
            t = {k: [] for k in runs}
            for _ in range(a.warmup):
                for fn in runs.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.reps):                                # alternating, so that drift hits all alike
                for k, fn in runs.items():
                    t[k].append(event_timed(fn))
            st = {k: stats(x) for k, x in t.items()}
            sz = torch.empty(0, dtype=dtype).element_size()
            lines.append(' %s, N = %d   (against form (a): kernels %.1e, form (b) %.1e)' % (str(dtype).split('.')[1], N, err[0], err[1]))
            for k in t:
                lines.append('  %-26s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((k,) + st[k]))
            k0, ka, kb = st['kernels (matvec + rank2)'], st['(a) V^T H V + outer'], st['(b) mv + 3 addr_']
            lines.append('  ratio (a) / kernels %.2f   (b) / kernels %.2f   larger IQR %.4f ms' % (ka[0] / k0[0], kb[0] / k0[0], max(k0[1], ka[1], kb[1])))
            lines.append('  kernels %.2f TB/s of %.1f MB; matvec pass %.2f TB/s of %.1f MB; rank2 pass %.2f TB/s of %.1f MB'
                         % (3 * N * N * sz / k0[0] / 1e9, 3 * N * N * sz / 1e6, N * N * sz / st['matvec pass'][0] / 1e9, N * N * sz / 1e6,
                            2 * N * N * sz / st['rank2 pass'][0] / 1e9, 2 * N * N * sz / 1e6))
            assert bool(torch.isfinite(Hw).all())
            del B, H0, Hk, Hr, Ht, Hw, eye
            torch.cuda.empty_cache()
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
