#!/usr/bin/env python3
"""
Lightcone sampling at the benchmark shape: 8 boxes of 256^3 float32, the 196 608 pixels of nside 128, 256 radii from
Cosmology().f2r over 100-200 MHz, 'linear' radial x 'linear' spatial interpolation.  The fused path (ONE launch of
rime_lcone_fwd through ops.lcone_sample) against two chains written with torch ops on the same GPU:
  (a) the reference's: per channel a whole interpolated cube b r + c over 256^3 voxels, then eight gathers and seven lerps;
  (b) gather first: per channel eight gathers from each of the two cubes, the lerps, then the radial combination.
Both chains are baselines, not the code under test.  All run in this process, alternating, after a warm-up; every repetition
is timed with device events.  Reported: median and spread of each, both ratios, the bytes per second of the fused launch
against its algorithmic traffic (the output written once, 2 x 8 voxels read per output) as a fraction of a copy_ of the same
number of bytes in this process, and whether two runs of each path gave the same bits.

  python tools/bench_lcone.py [--reps 20] [--warmup 2] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import cosmology, healpix, ops  # noqa: E402


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
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--nside', type=int, default=128)
    ap.add_argument('--box', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_lcone.py measures on the GPU; none found')
    assert a.reps >= 20
    dev = 'cuda:0'
    Nsim, N, Nr, res = 8, a.box, 256, 2.0
    g = torch.Generator(device=dev).manual_seed(3)
    boxes = torch.randn((Nsim, N, N, N), generator=g, device=dev, dtype=torch.float32)
    r = cosmology.Cosmology().f2r(np.linspace(100e6, 200e6, Nr))
    box_r = np.linspace(r.min(), r.max(), Nsim)
    vec = cosmology.unit_vectors(np.stack(healpix.pix2ang(a.nside)))
    Npix = vec.shape[1]
    idx, wgt, S = cosmology.radial_stencil(box_r, r, 'linear')
    dvec = torch.as_tensor(vec, device=dev)

    def fused():
        return ops.lcone_sample(boxes, r, idx, wgt, S, res, vec=dvec, interp='linear')

    def corners(dc):
        out = []
        for v in dvec:
            x = v * dc / res
            fl = torch.floor(x)
            i0 = torch.remainder(fl.long(), N)
            out.append((i0, torch.remainder(i0 + 1, N), (x - fl).float()))
        return out

    def trilinear(cube, c):
        (x0, x1, xd), (y0, y1, yd), (z0, z1, zd) = c
        c00 = cube[x0, y0, z0] * (1 - xd) + cube[x1, y0, z0] * xd
        c01 = cube[x0, y0, z1] * (1 - xd) + cube[x1, y0, z1] * xd
        c10 = cube[x0, y1, z0] * (1 - xd) + cube[x1, y1, z0] * xd
        c11 = cube[x0, y1, z1] * (1 - xd) + cube[x1, y1, z1] * xd
        return (c00 * (1 - yd) + c10 * yd) * (1 - zd) + (c01 * (1 - yd) + c11 * yd) * zd

    def chain_a():
        out = torch.empty((Nr, Npix), dtype=torch.float32, device=dev)
        for i in range(Nr):
            s1, s2 = int(idx[i, 0]), int(idx[i, 1])
            b = (boxes[s2] - boxes[s1]) / (box_r[s2] - box_r[s1])
            cube = b * r[i] + (boxes[s1] - b * box_r[s1])
            out[i] = trilinear(cube, corners(r[i]))
        return out

    def chain_b():
        out = torch.empty((Nr, Npix), dtype=torch.float32, device=dev)
        for i in range(Nr):
            c = corners(r[i])
            out[i] = float(wgt[i, 0]) * trilinear(boxes[idx[i, 0]], c) + float(wgt[i, 1]) * trilinear(boxes[idx[i, 1]], c)
        return out

    with torch.no_grad():
        yf, ya, yb = fused(), chain_a(), chain_b()
        scale = ya.abs().max()
        err_a, err_b = ((yf - ya).abs().max() / scale).item(), ((yf - yb).abs().max() / scale).item()
        assert err_b < 1e-5 and err_a < 1e-2, (err_a, err_b)            # (a) cancels r / dr ~ 70 eps in float32 per voxel
        same = {k: torch.equal(fn(), fn()) for k, fn in (('fused', fused), ('torch (a)', chain_a), ('torch (b)', chain_b))}
        nbytes = Nr * Npix * 4 * (1 + S * 8)
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        runs = {'fused launch': fused, 'torch chain (a)': chain_a, 'torch chain (b)': chain_b, 'copy (same bytes)': lambda: dst.copy_(src)}
        t = {k: [] for k in runs}
        for _ in range(a.warmup):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):                                          # alternating, so that drift hits all alike
            for k, fn in runs.items():
                t[k].append(timed(fn))
    s = {k: stats(v) for k, v in t.items()}
    lines = ['lightcone sampling, fused HIP launch vs two torch chains; %d boxes of %d^3 float32, nside %d (%d pixels), %d radii, '
             'linear x linear; %d reps after %d warm-up [ms]   (fused vs (a): %.1e, vs (b): %.1e of max)'
             % (Nsim, N, a.nside, Npix, Nr, a.reps, a.warmup, err_a, err_b)]
    for k in runs:
        lines.append('  %-19s median %10.4f   IQR %8.4f   min %10.4f   max %10.4f' % ((k,) + s[k]))
    f = s['fused launch']
    bw, cbw = nbytes / f[0] / 1e9, nbytes / s['copy (same bytes)'][0] / 1e9
    lines.append('  fused launch: %.3f TB/s of its algorithmic traffic (%.1f MB: output written once, %d voxels read per output); '
                 'copy_ of the same bytes (half read, half written): %.2f TB/s; fraction of the copy %.3f'
                 % (bw, nbytes / 1e6, S * 8, cbw, bw / cbw))
    for k in ('torch chain (a)', 'torch chain (b)'):
        c = s[k]
        lines.append('  ratio %s / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused faster beyond the spread: %s'
                     % (k, c[0] / f[0], c[0] - f[0], max(f[1], c[1]), (c[0] - f[0]) > max(f[1], c[1])))
    lines.append('  bit-identical across two runs: ' + ', '.join('%s %s' % kv for kv in same.items()))
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
