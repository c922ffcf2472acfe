#!/usr/bin/env python3
"""
Delay transform at the headline shape: visibilities (1, 1, 8128, 8, 256) complex64, FFT(dim=4, ndim=5, N=256, window='bh',
abs=True), the same with square=True, and PeakDelay.  The fused HIP path (fft.FFT -> ops.fft_apply, one launch) against the
reference's formulation written with torch ops on the same GPU (inp * win, torch.fft.fft, fftshift, abs, abs()**2:
fft.py:111-137).  The chain is the baseline, not the code under test.  Both run in this process, alternating, after a
warm-up, no gradient; every repetition is timed with device events; reported are the median and the spread of each, their
ratio, and the bytes per second of the fused launch against its algorithmic traffic (read the complex input once, write the
real output once).  PeakDelay is timed against the reference's per-line Python loop (fft.py:159-182, run on the chain's
output copied to the host as the reference would see a CPU tensor) on every 64th line; that time is multiplied by 64 and
labelled as extrapolated.

  python tools/bench_fft.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayeslim_amd import fft  # noqa: E402

NBL, NT, NF = 8128, 8, 256


def chain(win, square):
    def run(x):
        y = torch.fft.fftshift(torch.fft.fft(x * win, dim=4), dim=4)
        y = torch.abs(y)
        if square:
            y = torch.abs(y) ** 2
        return y
    return run


def timed(fn, x):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    ts = np.asarray(ts)
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return med, q3 - q1, ts.min(), ts.max()


def loop_peak(P, y):
    """the reference's PeakDelay loop on a host tensor of lines (L, N): get_peak once per line"""
    out = torch.zeros(len(y))
    for i in range(len(y)):
        line = y[i]
        n = torch.argmax(torch.abs(line))
        pos = n + 1 if n != len(line) - 1 else 0
        neg = n - 1 if n != 0 else -1
        rpos, rneg = torch.real(line[pos] / line[n]), torch.real(line[neg] / line[n])
        dpos, dneg = -rpos / (1 - rpos), rneg / (1 - rneg)
        out[i] = P.start + (n + ((dneg + dpos) / 2 + P.k(dneg ** 2) - P.k(dpos ** 2))) * P.df
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_fft.py measures on the GPU; none found')
    assert a.reps >= 20
    dev = 'cuda:0'
    rng = np.random.default_rng(13)
    x = torch.as_tensor(rng.normal(size=(1, 1, NBL, NT, NF)) + 1j * rng.normal(size=(1, 1, NBL, NT, NF)), dtype=torch.complex64,
                        device=dev)
    x = x + 4 * torch.exp(2j * np.pi * 37.3 * torch.arange(NF, device=dev) / NF).to(torch.complex64)
    lines = ['delay transform (1, 1, %d, %d, %d) complex64, window bh, fftshift; %d reps after %d warm-up, no gradient [ms]' % (
        NBL, NT, NF, a.reps, a.warmup)]
    with torch.no_grad():
        for square in (False, True):
            F = fft.FFT(dim=4, ndim=5, N=NF, window='bh', abs=True, square=square, device=dev)
            F.push(torch.float32)
            ref = chain(F.win, square)
            yf, yr = F(x), ref(x)
            err = ((yf - yr).abs().max() / yr.abs().max()).item()
            assert err < 1e-5, err                                 # two float32 transforms of the same data
            for _ in range(a.warmup):
                F(x)
                ref(x)
            torch.cuda.synchronize()
            t = {'fused': [], 'chain': []}
            for _ in range(a.reps):                                # alternating, so that drift hits both alike
                t['fused'].append(timed(F, x))
                t['chain'].append(timed(ref, x))
            sf, sc = stats(t['fused']), stats(t['chain'])
            nbytes = x.numel() * 8 + yf.numel() * 4
            lines.append(' abs=True%s' % (', square=True' if square else ''))
            for tag, s in (('fused', sf), ('chain', sc)):
                lines.append('  %-6s median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % ((tag,) + s))
            lines.append('  fused: %.2f TB/s of its algorithmic traffic (%.1f MB: input read once, output written once)' % (
                nbytes / sf[0] / 1e9, nbytes / 1e6))
            margin = sc[0] - sf[0]
            lines.append('  ratio chain / fused %.2f   median difference %.4f ms   larger IQR %.4f ms   fused vs chain: %.1e' % (
                sc[0] / sf[0], margin, max(sf[1], sc[1]), err))
            lines.append('  fused below chain by more than the larger spread: %s' % (margin > max(sf[1], sc[1])))
        # PeakDelay
        P = fft.PeakDelay(dim=4, ndim=5, N=NF, window='bh', device=dev)
        P.push(torch.float32)
        pk = P(x)
        for _ in range(a.warmup):
            P(x)
        torch.cuda.synchronize()
        sp = stats([timed(P, x) for _ in range(a.reps)])
        sub = torch.fft.fftshift(torch.fft.fft(x * P.win, dim=4), dim=4).reshape(-1, NF)[::64].cpu()
        t0 = time.perf_counter()
        ref = loop_peak(P, sub)
        tl = (time.perf_counter() - t0) * 1e3
        err = ((pk.reshape(-1)[::64].cpu() - ref).abs().max() / float(P.df)).item()
        lines.append(' PeakDelay (window bh), %d lines' % (NBL * NT))
        lines.append('  fused  median %9.4f   IQR %8.4f   min %9.4f   max %9.4f' % sp)
        lines.append('  reference loop on every 64th line (%d lines, host): %.1f ms; EXTRAPOLATED to all lines: %.0f ms' % (
            len(sub), tl, tl * 64))
        lines.append('  fused vs loop on those lines: %.1e df' % err)
    txt = '\n'.join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(txt + '\n')


if __name__ == '__main__':
    main()
