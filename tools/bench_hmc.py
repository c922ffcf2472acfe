#!/usr/bin/env python3
"""
One HMC trajectory at sampler sizes: the fused path (sampler._Trajectory: Nstep + 1 launches of rime_hmc_step, the last with
the kinetic energy, plus the energy-only pass for K_start) against the reference's operation chain written with torch ops on
the same tensors (leapfrog with a diagonal mass: p -= (eps / 2) g; then per step dq = c * p, dq = c * dq, q += dq * eps,
p -= eps * g; and K = sum((c * p)^2 / 2) twice).  The torch chain is the baseline, not the code under test.  A precomputed
gradient stands in for the potential in both (its copy into the gradient buffer is part of neither), so the figures are the
integrator's own cost.  Both run in this process, alternating, after a warm-up; a trajectory is timed with the host clock
between device synchronisations (both end in the read-back of the energy).  Reported: median and spread of each, their ratio,
and the bytes per second of the fused trajectory against its algorithmic traffic.

  float32, a diagonal mass, a per-element step size, Nstep = 10;  N = 786 432 (the C2 parameter count) and N = 2^24

  python tools/bench_hmc.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import sampler  # noqa: E402

NSTEP = 10


def torch_trajectory(q, p, g, eps, c):
    """the reference's leapfrog and kinetic energy, one torch op per operation of its code"""
    K0 = torch.sum((c * p) ** 2 / 2)
    p -= (eps / 2) * g
    for i in range(NSTEP):
        dq = c * p
        dq = c * dq
        q += dq * eps
        if i != NSTEP - 1:
            ge = eps * g
            p -= ge
    p -= (eps / 2) * g
    K1 = torch.sum((c * p) ** 2 / 2)
    return float(K0), float(K1)


def fused_trajectory(tr, eps, c):
    K0 = tr.kinetic(c)
    tr.stage(eps, c, 0.5, 1.0)
    for _ in range(NSTEP - 1):
        tr.stage(eps, c, 1.0, 1.0)
    return K0, tr.stage(eps, c, 0.5, 0.0, energy=True)


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


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
        sys.exit('bench_hmc.py measures on the GPU; none found')
    dev = 'cuda:0'
    gen = torch.Generator(device=dev).manual_seed(29)
    lines = ['HMC trajectory (Nstep = %d, diagonal mass, per-element eps), fused launches vs the reference chain in torch ops; '
             'float32, %d reps after %d warm-up [ms]' % (NSTEP, a.reps, a.warmup)]
    for N in (12288 * 64, 2 ** 24):
        rn = lambda: torch.randn(N, generator=gen, device=dev, dtype=torch.float32)
        q0, p0, g = rn(), rn(), rn() * 0.1
        eps = torch.rand(N, generator=gen, device=dev) * 0.01 + 0.005
        c = torch.rand(N, generator=gen, device=dev) + 0.5
        tr = sampler._Trajectory(sampler._Layout(q0))
        tr.g.copy_(g)
        qt, pt = q0.clone(), p0.clone()

        def reset():
            tr.q.copy_(q0), tr.p.copy_(p0), qt.copy_(q0), pt.copy_(p0)

        reset()
        Kf, Kt = fused_trajectory(tr, eps, c), torch_trajectory(qt, pt, g, eps, c)
        err = max(float((tr.q - qt).abs().max() / qt.abs().max()), float((tr.p - pt).abs().max() / pt.abs().max()),
                  abs(Kf[1] - Kt[1]) / abs(Kt[1]))
        runs = {'fused trajectory': lambda: fused_trajectory(tr, eps, c), 'torch chain': lambda: torch_trajectory(qt, pt, g, eps, c)}
        t = {k: [] for k in runs}
        for _ in range(a.warmup):
            for fn in runs.values():
                fn()
        for _ in range(a.reps):                                      # alternating, so that drift hits all alike
            reset()
            for k, fn in runs.items():
                t[k].append(host_timed(fn))
        st = {k: stats(x) for k, x in t.items()}
        lines.append(' N = %d   (fused vs torch, two float32 evaluations of q, p and K: %.1e)' % (N, err))
        for k in t:
            lines.append('  %-16s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((k,) + st[k]))
        f, b = st['fused trajectory'], st['torch chain']
        lines.append('  ratio torch / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused faster beyond the spread: %s'
                     % (b[0] / f[0], b[0] - f[0], max(f[1], b[1]), (b[0] - f[0]) > max(f[1], b[1])))
        # vectors moved: energy-only 2 (p, c); first and middle stages 7 (q, p, g, eps, c read, q, p written); last 5
        nbytes = (2 + 7 * NSTEP + 5) * N * 4
        lines.append('  fused trajectory %.2f TB/s of %.1f MB over %d launches' % (nbytes / f[0] / 1e9, nbytes / 1e6, NSTEP + 2))
        del tr, qt, pt, q0, p0, g, eps, c
        torch.cuda.empty_cache()
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
