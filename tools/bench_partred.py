#!/usr/bin/env python3
"""
The sparse mixing of calibration.PartialRedVisInflate at a HERA-like shape: the fused HIP path (ops.partred_inflate: one launch
forward, two fixed-order reductions backward) against the same mathematics written with torch ops on the same GPU:
  torch gather : index_select of the entries' model rows, multiply by c, index_add_ onto the output rows
  torch sparse : the reference's form (calibration.py:2307-2317): a CSR matrix built from c on every forward, the baseline axis
                 moved to the front, torch.sparse.mm on the real and on the imaginary plane, recombined
The torch forms are baselines, not the code under test.  All run in this process, alternating, after a warm-up; every
repetition is timed with device events; forward alone (no gradient) and forward plus backward (of Re sum(out * conj(cot)) for a
fixed cotangent, gradients of the data and of c).  A form that does not run here is reported with its error, not timed.
Reported: the median and spread of each, the ratios, each fused kernel alone with the bytes it moves (rows it reads, counted
once per read, plus what it writes) against its algorithmic minimum (every tensor once), both as a rate, the rate of a copy_ in
this process for scale, and whether two backward passes of each form gave the same bits.

Shape: Nout = 8128 physical baselines (the cross baselines of a 127-antenna hexagon plus one outrigger), Nin = 1600 redundant
models, 2 or 3 entries per baseline (20 % have 3) with distinct columns drawn near the baseline's own group, Npol = 1,
Nt = 60, Nf = 256, complex64: out is 1.0 GB.

  python tools/bench_partred.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import ops  # noqa: E402
from bayeslim_amd._lib import lib, check  # noqa: E402


def entries(Nout, Nin, rng):
    rows, cols = [], []
    for i in range(Nout):
        n = 3 if rng.uniform() < 0.2 else 2
        base = (i * Nin) // Nout
        js = (base + rng.choice(8, size=n, replace=False)) % Nin
        rows += [i] * n
        cols += [int(j) for j in js]
    return np.array(rows), np.array(cols)


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
    ap.add_argument('--nout', type=int, default=8128)
    ap.add_argument('--nin', type=int, default=1600)
    ap.add_argument('--nt', type=int, default=60)
    ap.add_argument('--nf', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_partred.py measures on the GPU; none found')
    dev = 'cuda:0'
    rng = np.random.default_rng(2178)
    Nout, Nin, Nt, Nf = a.nout, a.nin, a.nt, a.nf
    rows, cols = entries(Nout, Nin, rng)
    Nnz = len(rows)
    plan = ops.PartRedPlan(rows, cols, Nout, Nin)
    gen = torch.Generator(device=dev).manual_seed(5)
    cn = lambda *s: torch.complex(torch.randn(s, generator=gen, device=dev), torch.randn(s, generator=gen, device=dev))
    V, cot = cn(1, 1, Nin, Nt, Nf), cn(1, 1, Nout, Nt, Nf)
    c0 = torch.as_tensor(rng.uniform(0.2, 0.6, size=Nnz), dtype=torch.float32, device=dev)
    ri, ci = torch.as_tensor(rows, device=dev), torch.as_tensor(cols, device=dev)
    crow = torch.as_tensor(plan.roff, dtype=torch.int64, device=dev)

    def fused(v, c):
        return ops.partred_inflate(v, c, plan)

    def gather(v, c):
        out = torch.zeros((1, 1, Nout, Nt, Nf), dtype=v.dtype, device=dev)
        return out.index_add(2, ri, v.index_select(2, ci) * c[None, None, :, None, None])

    def sparse(v, c):                       # columns of a row must ascend in a CSR matrix: sort within the row, c along
        A = torch.sparse_csr_tensor(crow, ci[sp_order], c[sp_order], size=(Nout, Nin))
        d = v.moveaxis(2, 0)
        shape = d.shape
        d = d.reshape(shape[0], -1)
        re = torch.sparse.mm(A, d.real).reshape(Nout, *shape[1:]).moveaxis(0, 2)
        im = torch.sparse.mm(A, d.imag).reshape(Nout, *shape[1:]).moveaxis(0, 2)
        return torch.complex(re, im)

    sp_order = torch.as_tensor(np.lexsort((cols, rows)), device=dev)
    forms = {'fused': fused, 'torch gather': gather, 'torch sparse': sparse}

    def fwd_bwd(fn):
        def run():
            v, c = V.detach().requires_grad_(True), c0.detach().requires_grad_(True)
            (fn(v, c) * cot.conj()).real.sum().backward()
            return v.grad, c.grad
        return run

    lines = ['PartialRedVisInflate mixing, fused HIP path vs torch compositions; complex64, 1 pol; Nout %d, Nin %d, Nnz %d (rows of '
             '%d to %d entries, columns of up to %d), Nt %d, Nf %d; %d reps after %d warm-up [ms]'
             % (Nout, Nin, Nnz, int(np.diff(plan.roff).min()), plan.max_row, plan.max_col, Nt, Nf, a.reps, a.warmup)]
    with torch.no_grad():
        ref = fused(V, c0)
    gref = fwd_bwd(fused)()
    alive = {}
    for k, fn in forms.items():
        try:
            with torch.no_grad():
                y = fn(V, c0)
            g = fwd_bwd(fn)()
            g2 = fwd_bwd(fn)()
            err = [((x - r).abs().max() / r.abs().max()).item() for x, r in ((y, ref), (g[0], gref[0]), (g[1], gref[1]))]
            lines.append(' %-13s relative to fused: out %.1e  gdata %.1e  gc %.1e   backward bit-identical across two runs: %s'
                         % (k, err[0], err[1], err[2], torch.equal(g[0], g2[0]) and torch.equal(g[1], g2[1])))
            assert max(err) < 1e-3, (k, err)
            alive[k] = fn
            del y, g, g2
        except AssertionError:
            raise
        except Exception as e:                                           # a torch form that this build of torch cannot run
            if k == 'fused':
                raise
            lines.append(' %-13s did not run here: %s' % (k, str(e).splitlines()[0][:160]))
    # the three kernels alone, on contiguous operands
    code, NP = 0, 1
    T = plan.tables(dev)
    p = lambda t: ops._ptr(t)
    g = cot.contiguous()
    out, gV, gc = torch.empty_like(cot), torch.empty_like(V), torch.empty_like(c0)
    st = V.stride()
    dims = (Nout, Nin, Nnz, Nt, Nf)

    def k_fwd():
        check(lib.rime_partred_fwd(code, NP, ops._cptr(V), p(c0), p(T['roff']), p(T['col']), *dims, st[1], st[2], st[3], st[4],
                                   ops._cptr(out), ops._stream()), 'fwd')

    def k_data():
        check(lib.rime_partred_bwd_data(code, NP, ops._cptr(g), p(c0), p(T['row']), p(T['coff']), p(T['cmem']), *dims,
                                        ops._cptr(gV), ops._stream()), 'bwd_data')

    def k_coeff():
        check(lib.rime_partred_bwd_coeff(code, NP, ops._cptr(V), ops._cptr(g), p(T['roff']), p(T['col']), *dims, st[1], st[2], st[3],
                                         st[4], p(gc), ops._stream()), 'bwd_coeff')

    row = Nt * Nf * 8
    nchunk = int(np.sum(-(-np.diff(plan.roff) // 4)))
    traffic = {'kernel fwd': ((Nnz + Nout) * row, (Nin + Nout) * row),
               'kernel bwd_data': ((Nnz + Nin) * row, (Nout + Nin) * row),
               'kernel bwd_coeff': ((Nnz + nchunk) * row, (Nin + Nout) * row)}
    src = torch.empty(Nout * Nt * Nf, dtype=torch.complex64, device=dev).normal_()
    dst = torch.empty_like(src)
    runs = {}
    for k, fn in alive.items():
        runs[k + ' fwd'] = (lambda fn=fn: fn(V, c0))
        runs[k + ' fwd+bwd'] = fwd_bwd(fn)
    runs.update({'kernel fwd': k_fwd, 'kernel bwd_data': k_data, 'kernel bwd_coeff': k_coeff, 'copy of out': lambda: dst.copy_(src)})
    t = {k: [] for k in runs}
    for _ in range(a.warmup):
        for k, fn in runs.items():
            with torch.set_grad_enabled('+bwd' in k):
                fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):                                              # alternating, so that drift hits all alike
        for k, fn in runs.items():
            with torch.set_grad_enabled('+bwd' in k):
                t[k].append(timed(fn))
    s = {k: stats(v) for k, v in t.items()}
    for k in runs:
        lines.append('  %-22s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((k,) + s[k]))
    cbw = 2 * src.numel() * 8 / s['copy of out'][0] / 1e9
    lines.append('  copy_ of out (%.1f MB read + written): %.2f TB/s' % (2 * src.numel() * 8 / 1e6, cbw))
    for k, (moved, least) in traffic.items():
        lines.append('  %-17s moves %.1f MB (rows read, counted per read, + written) = %.2f TB/s; algorithmic minimum %.1f MB = %.2f '
                     'TB/s; moved / minimum %.2f' % (k, moved / 1e6, moved / s[k][0] / 1e9, least / 1e6, least / s[k][0] / 1e9, moved / least))
    for k in alive:
        if k == 'fused':
            continue
        for tag in ('fwd', 'fwd+bwd'):
            f, o = s['fused ' + tag], s[k + ' ' + tag]
            lines.append('  %-7s %s / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused faster beyond the spread: %s'
                         % (tag, k, o[0] / f[0], o[0] - f[0], max(f[1], o[1]), (o[0] - f[0]) > max(f[1], o[1])))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
