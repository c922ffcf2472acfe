"""
What the tests of the full-PSF kernel (csrc/psf.hip, ops.psf_gram) share: a float64 CPU restatement written from the
formula -- the fringe F[b, f, p] = exp(2 pi i nu_f / c  b_b . s_p) materialised with torch, then the einsum
    S[f, p, q] = Re sum_b conj(F[b, f, p]) w[b, f] F[b, f, q],      out[f, p, q] = rs[f, p] cs[f, q] S[f, p, q]
(with A = conj(F) beam this is the reference's A^T w conj(A), imaging.py:845-847) -- the random problems and the shape
tables.  No ops and no imaging product code in here.
"""
import numpy as np
import torch

C = 2.99792458e8
TOL = {'f64': 1e-10, 'f32': 2e-5}            # the imaging tolerances of this project (tests/test_rime_gpu.py:677)


def relmax(a, b):
    """max abs difference over max abs reference"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return np.abs(a - b).max() / np.abs(b).max()


def pointing_vectors(zen, az):
    """s = (sin z sin a, sin z cos a, cos z) of zenith angle / azimuth [deg]: (3, P) float64"""
    z, a = torch.deg2rad(torch.as_tensor(zen, dtype=torch.float64)), torch.deg2rad(torch.as_tensor(az, dtype=torch.float64))
    return torch.stack([torch.sin(z) * torch.sin(a), torch.sin(z) * torch.cos(a), torch.cos(z)])


def fringe(blvecs, s, freqs):
    """F (Nbl, Nf, P) complex128 of blvecs (Nbl, 3) [m], s (3, P), freqs (Nf,) [Hz]"""
    tau = torch.as_tensor(blvecs, dtype=torch.float64) @ torch.as_tensor(s, dtype=torch.float64)       # (Nbl, P) [m]
    ph = 2 * np.pi * torch.as_tensor(freqs, dtype=torch.float64)[None, :, None] / C * tau[:, None, :]
    return torch.polar(torch.ones_like(ph), ph)


def psf(blvecs, freqs, w, s, t=None, rs=None, cs=None):
    """the restatement: (Nf, P, Pq) float64; w (Nbl, Nf) or (Nbl, 1); t None: the rows again"""
    Fr = fringe(blvecs, s, freqs)
    Fq = Fr if t is None else fringe(blvecs, t, freqs)
    w = torch.as_tensor(w, dtype=torch.float64).expand(Fr.shape[0], Fr.shape[1])
    S = torch.einsum('bfp,bf,bfq->fpq', Fr.conj(), w.to(Fr.dtype), Fq).real
    if rs is not None:
        S = S * torch.as_tensor(rs, dtype=torch.float64)[:, :, None]
    if cs is not None:
        S = S * torch.as_tensor(cs, dtype=torch.float64)[:, None, :]
    return S


def problem(seed, Nbl, Nf, P, Pq=None, w_per_channel=True):
    """baselines up to 300 m at 150-250 MHz (phases of hundreds of turns), directions over the upper hemisphere, random
    positive w (Nbl, Nf) or (Nbl, 1), scales rs / cs in [0.5, 1.5]: a dict of float64 CPU tensors"""
    rng = np.random.default_rng(seed)
    blv = rng.uniform(-1, 1, (Nbl, 3)) * np.array([212.0, 212.0, 3.0])
    freqs = np.sort(rng.uniform(150e6, 250e6, Nf))                 # any channel grid

    def dirs(n):
        z, a = np.arccos(rng.uniform(0.1, 1.0, n)), rng.uniform(0, 2 * np.pi, n)
        return np.stack([np.sin(z) * np.sin(a), np.sin(z) * np.cos(a), np.cos(z)])

    out = dict(blvecs=blv, freqs=freqs, s=dirs(P), w=rng.uniform(0.2, 2.0, (Nbl, Nf if w_per_channel else 1)),
               rs=rng.uniform(0.5, 1.5, (Nf, P)), cs=rng.uniform(0.5, 1.5, (Nf, P if Pq is None else Pq)))
    if Pq is not None:
        out['t'] = dirs(Pq)
    return {k: torch.as_tensor(v, dtype=torch.float64) for k, v in out.items()}


def shapes(T, C, flush):
    """(P, Nbl, Nf, w per channel) of the symmetric-form cases: every P of {1, T-1, T, T+1, 2T+3}, every Nbl of
    {1, C-1, C+1, 2C+5} and both Nf at least once, the corner, and one sum longer than a flush interval"""
    return [(1, 1, 1, True), (T - 1, C - 1, 3, True), (T, C + 1, 1, False), (T + 1, 2 * C + 5, 1, True),
            (2 * T + 3, 1, 3, False), (2 * T + 3, 2 * C + 5, 3, True), (T + 1, C - 1, 3, False), (5, flush + C + 3, 1, True)]


def rect_shapes(T):
    """(P, Pq) of the rectangular-form cases"""
    return [(T + 1, 1), (T + 1, T - 1), (T + 1, 2 * T + 3)]
