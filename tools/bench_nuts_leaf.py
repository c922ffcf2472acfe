#!/usr/bin/env python3
"""
One leaf of the NUTS tree at a sampler size: the two fused launches of csrc/nuts.hip (nuts.leaf_open, nuts.leaf_close with the
kinetic energy and the two projections of the no-U-turn criterion, and the readback of the three doubles) against the same leaf
composed from the pieces the package had before them: two clones of the edge state, two launches of sampler.hmc_step (the second
with the energy), sampler.hoffman_uturn on the four vectors, and the readback of the energy.  The composition is the baseline,
not the code under test.  A precomputed gradient stands in for the potential in both (its evaluation and its pack into the flat
buffer are the same in both and part of neither), so the figures are the leaf's own passes.  Both allocate their outputs as the
sampler does (fresh q and p per leaf).  Both run in this process, alternating, after a warm-up; a leaf is timed with the host
clock between device synchronisations.  Reported: median and spread of each, their ratio, and the bytes per second of the fused
leaf against its algorithmic traffic.

  float32, a diagonal mass (c a vector), a scalar step size;  N = 2^22

  python tools/bench_nuts_leaf.py [--reps 50] [--warmup 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import nuts, sampler  # noqa: E402

N = 2 ** 22
H = 0.01


def fused_leaf(q0, p0, g0, g1, c, q_far, p_far, out, ws):
    q1, p1 = torch.empty_like(q0), torch.empty_like(p0)
    nuts.leaf_open(q0, p0, g0, q1, p1, None, c, H)
    nuts.leaf_close(q1, p1, g1, None, c, H, q_far, p_far, out, ws)
    K, far, near = out.tolist()
    return q1, p1, K, (far < 0) or (near < 0)


def composed_leaf(q0, p0, g0, g1, c, q_far, p_far, energy, ws):
    q1, p1 = q0.clone(), p0.clone()
    sampler.hmc_step(q1, p1, g0, None, c, H / 2, H)
    sampler.hmc_step(None, p1, g1, None, c, H / 2, 0.0, energy, ws)
    turning = sampler.hoffman_uturn(q_far, q1, p_far, p1)
    return q1, p1, float(energy), turning


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
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_nuts_leaf.py measures on the GPU; none found')
    dev = 'cuda:0'
    gen = torch.Generator(device=dev).manual_seed(31)
    rn = lambda: torch.randn(N, generator=gen, device=dev, dtype=torch.float32)
    q0, p0, g0, g1, q_far, p_far = rn(), rn(), rn() * 0.1, rn() * 0.1, rn(), rn()
    c = torch.rand(N, generator=gen, device=dev) + 0.5
    out = torch.zeros(3, dtype=torch.float64, device=dev)
    energy = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.empty(int(nuts._lib.lib.rime_nuts_workspace(N)) // 8, dtype=torch.float64, device=dev)
    runs = {'fused leaf': lambda: fused_leaf(q0, p0, g0, g1, c, q_far, p_far, out, ws),
            'composed leaf': lambda: composed_leaf(q0, p0, g0, g1, c, q_far, p_far, energy, ws)}
    f, b = runs['fused leaf'](), runs['composed leaf']()
    same = torch.equal(f[0], b[0]) and torch.equal(f[1], b[1]) and f[2] == b[2] and f[3] == b[3]
    t = {k: [] for k in runs}
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    for _ in range(a.reps):                                          # alternating, so that drift hits both alike
        for k, fn in runs.items():
            t[k].append(host_timed(fn))
    st = {k: stats(x) for k, x in t.items()}
    lines = ['NUTS leaf (diagonal mass, scalar step), two fused launches vs clones + two rime_hmc_step + hoffman_uturn in torch; '
             'float32, N = %d, %d reps after %d warm-up [ms]' % (N, a.reps, a.warmup),
             ' q, p and the kinetic energy bit-identical, the same criterion: %s' % same]
    for k in t:
        lines.append('  %-14s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((k,) + st[k]))
    fs, bs = st['fused leaf'], st['composed leaf']
    lines.append('  ratio composed / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused faster beyond the spread: %s'
                 % (bs[0] / fs[0], bs[0] - fs[0], max(fs[1], bs[1]), (bs[0] - fs[0]) > max(fs[1], bs[1])))
    # vectors moved by the fused leaf: open reads q0, p0, g0, c and writes q1, p1 (6); close reads p1, g1, c, q1, q_far, p_far
    # and writes p1 (7)
    nbytes = 13 * N * 4
    lines.append('  fused leaf %.2f TB/s of %.1f MB over 3 launches' % (nbytes / fs[0] / 1e9, nbytes / 1e6))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
