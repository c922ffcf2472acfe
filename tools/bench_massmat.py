#!/usr/bin/env python3
"""
One leapfrog stage and one NUTS leaf with a dense mass on the launches of csrc/massmat.hip (massmat.project, massmat.drift) against
the same arithmetic in torch ops: L^T @ p and L @ z as full-matrix mat-vecs, the elementwise kick and drift, sum(z^2) and the two
dot products of the no-U-turn criterion.  The torch chain is the baseline, not the code under test.  A precomputed gradient stands
in for the potential in both.  Both run in this process, alternating, after a warm-up; a call is timed with the host clock between
device synchronisations, `inner` calls per timing so that a timing is not one launch latency.  Reported per case: median and spread
of each, their ratio, whether the fused path is faster beyond the spread, and the bytes per second of the fused stage against the
factor's triangle, n (n + 1) / 2 sizeof(T) per triangular launch (two per stage).

  cases: one block n = 1024 and n = 4096, float32 and float64; a mixed layout (diagonal 4096 + dense real 1024 + dense complex 512)

  python tools/bench_massmat.py [--reps 30] [--warmup 5] [--inner 10] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import massmat  # noqa: E402

H = 0.01
DEV = 'cuda:0'


class Case:
    """flat vectors of one layout: blocks = [(n, off, nrhs)], diagonal elsewhere"""

    def __init__(self, name, dtype, blocks, N, gen):
        self.name, self.dtype, self.N = name, dtype, N
        rn = lambda *s: torch.randn(*s, generator=gen, device=DEV, dtype=dtype)
        self.L = [torch.eye(n, device=DEV, dtype=dtype) + 0.3 * torch.tril(rn(n, n)) / n ** 0.5 for n, _, _ in blocks]
        self.blocks = blocks
        self.table, self.keep = massmat.make_table([(L, off, nrhs) for L, (_, off, nrhs) in zip(self.L, blocks)], N, dtype, DEV)
        self.q, self.p, self.g0, self.g1, self.q_far, self.p_far = rn(N), rn(N), 0.1 * rn(N), 0.1 * rn(N), rn(N), rn(N)
        self.c = torch.rand(N, generator=gen, device=DEV, dtype=dtype) + 0.5
        self.z, self.p2, self.q2 = torch.empty_like(self.p), torch.empty_like(self.p), torch.empty_like(self.p)
        self.out = torch.zeros(3, dtype=torch.float64, device=DEV)
        self.ws = torch.empty(int(massmat._lib.lib.rime_mass_workspace(N)) // 8, dtype=torch.float64, device=DEV)
        cover = torch.zeros(N, dtype=torch.bool, device=DEV)
        for n, off, nrhs in blocks:
            cover[off:off + n * nrhs] = True
        self.diag = ~cover
        self.tri_bytes = sum(n * (n + 1) // 2 for n, _, _ in blocks) * self.L[0].element_size()

    # ---- the fused launches
    def fused_stage(self):
        massmat.project(self.table, self.p, self.g0, None, self.c, H, self.p2, self.z)
        massmat.drift(self.table, self.z, self.q, None, self.c, H, self.q2)
        return self.q2, self.p2

    def fused_leaf(self):
        q1, ph, p1 = torch.empty_like(self.q), torch.empty_like(self.p), torch.empty_like(self.p)
        massmat.project(self.table, self.p, self.g0, None, self.c, H / 2, ph, self.z)
        massmat.drift(self.table, self.z, self.q, None, self.c, H, q1)
        massmat.project(self.table, ph, self.g1, None, self.c, H / 2, p1, self.z)
        massmat.drift(self.table, self.z, q1, None, self.c, 0.0, None, p=p1, q_far=self.q_far, p_far=self.p_far, out=self.out, ws=self.ws)
        K, far, near = self.out.tolist()
        return q1, p1, K, (far < 0) or (near < 0)

    # ---- the same in torch ops
    def _z(self, p):
        z = self.c * p
        for L, (n, off, nrhs) in zip(self.L, self.blocks):
            z[off:off + n * nrhs] = (L.T @ p[off:off + n * nrhs].view(n, nrhs)).reshape(-1)
        return z

    def _y(self, z):
        y = self.c * z
        for L, (n, off, nrhs) in zip(self.L, self.blocks):
            y[off:off + n * nrhs] = (L @ z[off:off + n * nrhs].view(n, nrhs)).reshape(-1)
        return y

    def torch_stage(self):
        p = self.p - H * self.g0
        return self.q + H * self._y(self._z(p)), p

    def torch_leaf(self):
        ph = self.p - (H / 2) * self.g0
        q1 = self.q + H * self._y(self._z(ph))
        p1 = ph - (H / 2) * self.g1
        z = self._z(p1)
        d = q1 - self.q_far
        K, far, near = torch.stack([0.5 * (z * z).sum(), d @ self.p_far, d @ p1]).tolist()
        return q1, p1, K, (far < 0) or (near < 0)


def host_timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def stats(ts):
    q1, med, q3 = np.percentile(np.asarray(ts), [25, 50, 75])
    return med, q3 - q1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_massmat.py measures on the GPU; none found')
    gen = torch.Generator(device=DEV).manual_seed(47)
    cases = []
    for dtype in (torch.float32, torch.float64):
        tag = 'f32' if dtype == torch.float32 else 'f64'
        for n in (1024, 4096):
            cases.append(Case('n = %d %s' % (n, tag), dtype, [(n, 0, 1)], n, gen))
        cases.append(Case('mixed 4096 + 1024 + 2 x 512 %s' % tag, dtype, [(1024, 4096, 1), (512, 5120, 2)], 6144, gen))
    lines = ['dense-mass leapfrog stage and NUTS leaf: the launches of csrc/massmat.hip vs torch ops (two full mat-vecs, elementwise '
             'ops, reductions); %d reps of %d calls after %d warm-up; ms per call, median (IQR)' % (a.reps, a.inner, a.warmup)]
    for cs in cases:
        u = 2.0 ** -24 if cs.dtype == torch.float32 else 2.0 ** -53
        f, t = cs.fused_stage(), cs.torch_stage()
        err = max(float((f[0] - t[0]).abs().max()), float((f[1] - t[1]).abs().max()))
        lf, lt = cs.fused_leaf(), cs.torch_leaf()
        same = lf[3] == lt[3] and abs(lf[2] - lt[2]) <= 1e3 * u * abs(lt[2])
        runs = {'fused stage': cs.fused_stage, 'torch stage': cs.torch_stage, 'fused leaf': cs.fused_leaf, 'torch leaf': cs.torch_leaf}
        ts = {k: [] for k in runs}
        for _ in range(a.warmup):
            for fn in runs.values():
                fn()
        for _ in range(a.reps):                                          # alternating, so that drift hits all alike
            for k, fn in runs.items():
                ts[k].append(host_timed(fn, a.inner))
        st = {k: stats(v) for k, v in ts.items()}
        lines.append('%s   (stage: max |fused - torch| %.2e; leaf: same criterion and energy: %s)' % (cs.name, err, same))
        for what in ('stage', 'leaf'):
            fs, bs = st['fused ' + what], st['torch ' + what]
            lines.append('  %-5s fused %8.4f (%6.4f)   torch %8.4f (%6.4f)   torch / fused %5.2f   fused faster beyond the spread: %s'
                         % (what, fs[0], fs[1], bs[0], bs[1], bs[0] / fs[0], (bs[0] - fs[0]) > max(fs[1], bs[1])))
        # a stage streams the triangle twice (L^T p, L z); a leaf three times (the last drift has drift = 0)
        lines.append('  triangle %.2f MB per launch: the fused stage moves it at %.3f TB/s (host time of the whole stage, launches included)'
                     % (cs.tri_bytes / 1e6, 2 * cs.tri_bytes / st['fused stage'][0] / 1e9))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
