#!/usr/bin/env python3
"""
The redundant-visibility term at the shapes redundant calibration uses it: the fused HIP path (ops.redvis: one launch forward,
one segmented fixed-order reduction backward) against the reference's expression written with torch ops on the same GPU
(index_select along the baseline axis + add, calibration.py:989-997; autograd's backward of index_select is an atomic
scatter-add).  The torch chain is the baseline, not the code under test.  Both run in this process, alternating, after a
warm-up; every repetition is timed with device events; forward alone (no gradient) and forward plus backward (of
Re sum(out * conj(cot)) for a fixed cotangent).  Reported: the median and spread of each, their ratio, the bytes per second of
the fused forward and backward against their algorithmic traffic as a fraction of what a copy_ of the same number of bytes
reaches in this process, the time of the backward kernel alone against a copy of gout, and whether two backward passes of each
path gave the same bits.

  (a) the headline array: 127-antenna hexagon + outrigger, 8128 cross baselines grouped by build_reds; 8 times, 256 channels, 1 pol
  (b) 37-antenna hexagon, 666 cross baselines; 60 times, 128 channels, 1 pol

  python tools/bench_redcal.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import ops, telescope_model, utils  # noqa: E402


def grouping(N, outrigger):
    ants, vecs = utils._make_hex(N, D=14.6)
    if outrigger:
        ants, vecs = list(ants) + [len(ants)], np.vstack([vecs, [[383.7, -211.3, 0.0]]])
    antpos = utils.AntposDict(ants, vecs)
    bls = [(a, b) for i, a in enumerate(ants) for b in ants[i + 1:]]
    reds, _, bl2red = telescope_model.build_reds(antpos, bls=bls)[:3]
    return np.array([bl2red[b] for b in bls]), len(reds)


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
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_redcal.py measures on the GPU; none found')
    assert a.reps >= 20
    dev = 'cuda:0'
    rng = np.random.default_rng(23)
    cn = lambda *s: torch.complex(torch.as_tensor(rng.normal(size=s), dtype=torch.float32, device=dev),
                                  torch.as_tensor(rng.normal(size=s), dtype=torch.float32, device=dev))
    cases = [('(a) hex-127 + outrigger, 8128 baselines, 8 times, 256 channels', 7, True, 8, 256),
             ('(b) hex-37, 666 baselines, 60 times, 128 channels', 4, False, 60, 128)]
    lines = ['RedVisModel term, fused HIP path vs index_select + add in torch; complex64, 1 pol; %d reps after %d warm-up [ms]'
             % (a.reps, a.warmup)]
    for name, N, outr, Nt, Nf in cases:
        red, Nred = grouping(N, outr)
        Nbl = len(red)
        sizes = np.bincount(red)
        plan = ops.RedVisPlan(red, Nred, Ntm=Nt)
        idx = torch.as_tensor(red, device=dev)
        vis, model, cot = cn(1, 1, Nbl, Nt, Nf), cn(1, 1, Nred, Nt, Nf), cn(1, 1, Nbl, Nt, Nf)
        fused = lambda m: ops.redvis(vis, m, plan)
        chain = lambda m: vis + torch.index_select(m, -3, idx)

        def fwd_bwd(fn):
            def run():
                m = model.detach().requires_grad_(True)
                (fn(m) * cot.conj()).real.sum().backward()
                return m.grad
            return run

        with torch.no_grad():
            yf, yr = fused(model), chain(model)
        assert torch.equal(yf, yr)                                       # one rounding of the same sum on either path
        gf, gr = fwd_bwd(fused)(), fwd_bwd(chain)()
        err = ((gf - gr).abs().max() / gr.abs().max()).item()
        assert err < 1e-4, (name, err)
        same = {k: torch.equal(fwd_bwd(fn)(), fwd_bwd(fn)()) for k, fn in (('fused', fused), ('torch', chain))}
        gout, gdst = cot.contiguous(), torch.empty_like(cot)
        fbytes = (2 * vis.numel() + model.numel()) * 8                   # vis read, out written, model read once
        bbytes = (gout.numel() + model.numel()) * 8                      # gout read once, gmodel written once
        bufs = {}
        for tag, nb in (('fwd', fbytes), ('bwd', bbytes)):
            src = torch.empty(nb // 8, dtype=torch.float32, device=dev).normal_()
            bufs[tag] = (src, torch.empty_like(src))
        runs = {'fused fwd': lambda: fused(model), 'torch fwd': lambda: chain(model),
                'copy (fwd bytes)': lambda: bufs['fwd'][1].copy_(bufs['fwd'][0]),
                'fused fwd+bwd': fwd_bwd(fused), 'torch fwd+bwd': fwd_bwd(chain),
                'fused bwd kernel': lambda: ops._redvis_bwd_call(plan, gout, 1),
                'copy (bwd bytes)': lambda: bufs['bwd'][1].copy_(bufs['bwd'][0]),
                'copy of gout': lambda: gdst.copy_(gout)}
        t = {k: [] for k in runs}
        for _ in range(a.warmup):
            for k, fn in runs.items():
                with torch.set_grad_enabled('+bwd' in k):
                    fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):                                          # alternating, so that drift hits all alike
            for k, fn in runs.items():
                with torch.set_grad_enabled('+bwd' in k):
                    t[k].append(timed(fn))
        s = {k: stats(v) for k, v in t.items()}
        lines.append(' %s: %d groups, members per group median %d, max %d   (fused vs torch gradient: %.1e)'
                     % (name, Nred, int(np.median(sizes)), int(sizes.max()), err))
        for k in runs:
            lines.append('  %-17s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((k,) + s[k]))
        for tag, key, nb, ck in (('fwd', 'fused fwd', fbytes, 'copy (fwd bytes)'), ('bwd kernel', 'fused bwd kernel', bbytes, 'copy (bwd bytes)')):
            bw, cbw = nb / s[key][0] / 1e9, nb / s[ck][0] / 1e9
            lines.append('  fused %s: %.2f TB/s of its algorithmic traffic (%.1f MB); copy_ of the same bytes (half read, half '
                         'written): %.2f TB/s; fraction %.2f' % (tag, bw, nb / 1e6, cbw, bw / cbw))
        lines.append('  fused bwd kernel / copy of gout: %.2f' % (s['fused bwd kernel'][0] / s['copy of gout'][0]))
        for tag in ('fwd', 'fwd+bwd'):
            f, c = s['fused ' + tag], s['torch ' + tag]
            lines.append('  %-7s ratio torch / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused faster beyond the '
                         'spread: %s' % (tag, c[0] / f[0], c[0] - f[0], max(f[1], c[1]), (c[0] - f[0]) > max(f[1], c[1])))
        lines.append('  backward bit-identical across two runs: fused %s, torch %s' % (same['fused'], same['torch']))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
