#!/usr/bin/env python3
"""
The mutual-coupling term at the shape the calibration chain uses it: the fused HIP path (ops.coupling_apply: the visibility
matrix read through a table, E = I + X o D built on the fly, only the output baselines written; the backward recomputes
T = E V) against the reference's op chain restated with torch ops on the same GPU (index_select to (Nant^2, Nt, Nf), null,
conjugate, two einsums over the antenna axes, index_select back; calibration.py:1497-1539, autograd keeps its
intermediates).  The torch chain is the baseline, not the code under test.  Both run in this process, alternating, after a
warm-up; every repetition of forward plus backward (of Re sum(out * conj(cot)) for a fixed cotangent) is timed with device
events, and the peak of the allocator over one repetition of each path is read after a reset of its statistics.  Reported:
the median and spread of each, their ratio, the peak memory above the inputs, and whether two runs of each path gave both
gradients with the same bits.

  HERA-128: 128 antennas, 8128 cross baselines (the auto-correlations are null), 8 times, 256 channels, complex64;
  the coupling per time (Tm = Nt) and one for all times (Tm = 1)

  python tools/bench_coupling.py [--reps 10] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import ops  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stats(ts):
    ts = np.asarray(ts)
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return dict(median_ms=float(med), iqr_ms=float(q3 - q1), min_ms=float(ts.min()), max_ms=float(ts.max()))


def tables(N):
    """cross baselines of N antennas numbered in matrix order: (plan table, out_rows, and the reference's index tensors)"""
    C = ops.COUPLING_CONJ
    table = np.full((N, N), -1, dtype=np.int64)
    iu = np.triu_indices(N, 1)
    rows = np.arange(len(iu[0]))
    table[iu] = rows
    table[iu[1], iu[0]] = rows | C
    out_rows = iu[0] * N + iu[1]
    flat_idx = np.where(table < 0, 0, table & (C - 1)).reshape(-1)
    null = (table < 0).reshape(-1)
    conj = ((table >= 0) & ((table & C) != 0)).reshape(-1)
    return table, out_rows, flat_idx, null, conj


def torch_chain(X, D, data, I, flat_idx, null, conj, bls_idx, N):
    """the reference's forward, op for op, out of place where it writes in place"""
    coupling = X * D + I
    flat = torch.index_select(data, 0, flat_idx)
    flat = torch.where(null[:, None, None], torch.zeros((), dtype=flat.dtype, device=flat.device), flat)
    flat = torch.where(conj[:, None, None], flat.conj(), flat)
    V = flat.reshape((N, N) + data.shape[1:])
    V = torch.einsum('patf,aqtf->pqtf', coupling, V)
    V = torch.einsum('patf,qatf->pqtf', V, coupling.conj())
    return torch.index_select(V.flatten(0, 1), 0, bls_idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    N, Nt, Nf = 128, 8, 256
    rng = np.random.default_rng(0)
    table, out_rows, flat_idx, null, conj = tables(N)
    Nbl = len(out_rows)
    plan = ops.CouplingPlan(table, out_rows, Nbl)
    cx = lambda *s: torch.as_tensor(rng.normal(size=s) + 1j * rng.normal(size=s)).to(torch.complex64).to(dev)
    data0, cot = cx(Nbl, Nt, Nf), cx(Nbl, Nt, Nf)
    D = torch.exp(1j * torch.as_tensor(rng.uniform(0, 2 * np.pi, size=(N, N, 1, Nf)))).to(torch.complex64).to(dev)
    I = torch.eye(N, device=dev)[:, :, None, None]
    T = lambda x: torch.as_tensor(x, device=dev)
    flat_idx, null, conj, bls_idx = T(flat_idx), T(null), T(conj), T(out_rows)
    result = dict(shape=dict(N=N, Nbl=Nbl, Nt=Nt, Nf=Nf, dtype='complex64'), device=torch.cuda.get_device_name(0), cases={})
    for tag, Tm in (('Tm=Nt', Nt), ('Tm=1', 1)):
        X0 = 0.05 * cx(N, N, Tm, Nf)

        def step(path):
            X, data = X0.clone().requires_grad_(True), data0.clone().requires_grad_(True)
            if path == 'fused':
                W = ops.coupling_apply(X, D, data, plan, add_I=True, prod='both')
            else:
                W = torch_chain(X, D, data, I, flat_idx, null, conj, bls_idx, N)
            (W * cot.conj()).real.sum().backward()
            return W.detach(), X.grad, data.grad

        times, peaks, same, outs = {'fused': [], 'torch': []}, {}, {}, {}
        for path in ('fused', 'torch'):
            for _ in range(a.warmup):
                step(path)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            first = step(path)
            torch.cuda.synchronize()
            peaks[path] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            second = step(path)
            same[path] = bool(torch.equal(first[1], second[1]) and torch.equal(first[2], second[2]))
            outs[path] = first
            del second
        for _ in range(a.reps):
            for path in ('fused', 'torch'):
                times[path].append(timed(lambda: step(path))[0])
        scale = [float(o.abs().max()) for o in outs['torch']]
        diff = [float((f - t).abs().max()) / s for f, t, s in zip(outs['fused'], outs['torch'], scale)]
        case = dict(fused=stats(times['fused']), torch=stats(times['torch']), peak_MiB=peaks, bit_identical_gradients=same,
                    max_rel_difference=dict(W=diff[0], gX=diff[1], gdata=diff[2]))
        case['torch_over_fused'] = case['torch']['median_ms'] / case['fused']['median_ms']
        result['cases'][tag] = case
        print('%-6s fused %8.2f ms (iqr %.2f)  torch %8.2f ms (iqr %.2f)  torch / fused %.2f  peak MiB fused %.0f torch %.0f  '
              'same bits fused %s torch %s  max rel diff W %.1e gX %.1e gdata %.1e'
              % (tag, case['fused']['median_ms'], case['fused']['iqr_ms'], case['torch']['median_ms'], case['torch']['iqr_ms'],
                 case['torch_over_fused'], peaks['fused'], peaks['torch'], same['fused'], same['torch'], *diff), flush=True)
        del outs
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
