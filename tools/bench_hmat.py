#!/usr/bin/env python3
"""
Times the fused operator apply (hmat plan, csrc/hmat.hip) against the same tree applied leaf by leaf in torch ops, both
alternating in one process (the method of bench_lbfgs.py), on a partitioned Hessian shaped like the headline fit's parameter
groups: a few dense blocks, a long diagonal-plus-low-rank block and low-rank couplings.  Also the L-BFGS direction at m = 10 / 100
with that starting matrix.  Prints one JSON line with times and achieved bytes per second; no number gates anything.

Usage:  python tools/bench_hmat.py [--nsky 1000000] [--rank 32] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayeslim_amd import hmat, bfgs   # noqa: E402


def leafwise(blocks, x, sizes):
    """the reference's evaluation order in torch ops: one or two matmuls per leaf, glued with cat"""
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    out = [torch.zeros(n, dtype=x.dtype, device=x.device) for n in sizes]
    for (i, j), leaf in blocks.items():
        for (a, b, t) in (((i, j, False),) if i == j else ((i, j, False), (j, i, True))):
            xs = x[offs[b - 1]:offs[b]]
            if isinstance(leaf, hmat.DenseMat):
                out[a - 1] += (leaf.H.T if t else leaf.H) @ xs
            else:
                U, V = leaf.U, (leaf.U.T if leaf.hermitian else leaf.V)
                out[a - 1] += (V.T @ (U.T @ xs)) if t else (U @ (V @ xs))
                if leaf.Hdiag is not None:
                    out[a - 1] += leaf.Hdiag * xs
    return torch.cat(out)


def timed(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nsky', type=int, default=1000000)
    ap.add_argument('--rank', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    dev, dt = 'cuda:0', torch.float32
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=dt)
    sizes = [2048, 1024, args.nsky]
    blocks = {(1, 1): hmat.DenseMat(rnd(2048, 2048)), (2, 2): hmat.DenseMat(rnd(1024, 1024)),
              (3, 3): hmat.SparseMat((args.nsky, args.nsky), rnd(args.nsky, args.rank) / 30, Hdiag=torch.rand(args.nsky, generator=g, device=dev) + 0.5,
                                     hermitian=True),
              (1, 2): hmat.DenseMat(rnd(2048, 1024)), (1, 3): hmat.SparseMat((2048, args.nsky), rnd(2048, 8), V=rnd(8, args.nsky) / 30)}
    P = hmat.PartitionedMat(dict(blocks), symmetric=True)
    N = sum(sizes)
    x = rnd(N)
    nbytes = 4 * (2048 * 2048 + 1024 * 1024 + 2 * 2048 * 1024 + 2 * args.nsky * args.rank + args.nsky + 2 * 8 * (2048 + args.nsky) + 2 * N)
    y0, y1 = P(x), leafwise(blocks, x, sizes)
    res = dict(N=N, rank=args.rank, rel_diff=float((y0 - y1).abs().max() / y1.abs().max()), fused_s=[], torch_s=[])
    for _ in range(3):                                    # alternate: drift hits both alike
        res['fused_s'].append(timed(lambda: P(x), args.reps))
        res['torch_s'].append(timed(lambda: leafwise(blocks, x, sizes), args.reps))
    res['fused_bytes_per_s'] = nbytes / min(res['fused_s'])
    res['torch_bytes_per_s'] = nbytes / min(res['torch_s'])
    for m in (10, 100):
        s = [rnd(N) for _ in range(m)]
        y = [si * 1.5 + 0.1 * rnd(N) for si in s]
        rho = [1.0 / float(a @ b) for a, b in zip(s, y)]
        bfgs.two_loop_recursion(x, s, y, rho, H0=P)
        res['direction_m%d_s' % m] = timed(lambda: bfgs.two_loop_recursion(x, s, y, rho, H0=P), 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
