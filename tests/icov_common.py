"""
Shared by test_icov_host.py and test_icov_gpu.py: the cases of the axis covariances (optim.apply_icov, ops.chisq_axis), their
seeded inputs, the float64 oracle and the error bound.

Oracle: the reference's own branches cannot run (they name an undefined variable), so the oracle is a float64 CPU
evaluation of the einsums tabulated in DESIGN.md ("Axis covariances"), written here independently of bayeslim_amd, and cross-checked in the host test against a
plain Python loop over batches (r.conj() @ W[b] @ r).

Inputs: W = A A^H + n I per batch from a seeded generator (Hermitian, positive definite, well conditioned), pred and data of
order one.  They are rounded to the precision under test FIRST; the oracle works on those rounded values in float64.

Error bound |err| <= C_ORDER (2 n + 8) u S, S = sum_ab |r_a| |W_ab| |r_b| (per batch for q, summed for the total; per
element of y with sum_c |W_ac| |r_c| in place of S), u = 2^-24 (complex64) or 2^-53 (complex128).  Where C_ORDER comes from:
one row product y_a = sum_c W_ac r_c is, per real component, a sum of 2 n real products (fused multiply-adds), whatever the
order: each lane of the row's group chains its share, the partial sums are added in a shuffle tree.  ANY order of 2 n terms
has |error| <= gamma_2n sum |terms| (Higham, Accuracy and Stability, 4.2) with gamma_2n ~ 2 n u, and per component
sum_c (|Wr rr| + |Wi ri|) <= sum_c |W_ac| |r_c| (Cauchy-Schwarz), so the complex error is at most
sqrt(2) (2 n) u sum_c |W_ac| |r_c|.  The tree only shortens the chains, so the order actually used stays within that.  The
remaining roundings are a fixed number: r = pred - data (u per component, twice: in y and in the closing product), the
closing product conj(r_a) y_a and the sums across rows and work-groups in double (nothing at this scale), the conversion
of q or of the total to the output precision (u), and in the backward the scaling by 2 g (u): fewer than 8 u in all.  So
sqrt(2) (2 n + 8) u S bounds it; C_ORDER = 2 rounds sqrt(2) up and absorbs the second-order terms.  It is not fitted to
what the kernel returns.
"""
import functools

import numpy as np
import torch

C_ORDER = 2.0
UNIT = {torch.complex64: 2.0 ** -24, torch.complex128: 2.0 ** -53}

# (mode, cov_axis, data shape, icov shape, output shape, einsum), as DESIGN.md ("Axis covariances") tabulates them
VIS, MAP = (2, 2, 5, 4, 6), (2, 1, 6, 7)
CASES = [
    ('vis', 'bl', VIS, (2, 2, 4, 6, 5, 5), (2, 2, 4, 6), 'ijklm,ijlmkn,ijnlm->ijlm'),
    ('vis', 'time', VIS, (2, 2, 5, 6, 4, 4), (2, 2, 5, 6), 'ijklm,ijkmln,ijknm->ijkm'),
    ('vis', 'freq', VIS, (2, 2, 5, 4, 6, 6), (2, 2, 5, 4), 'ijklm,ijklmn,ijkln->ijkl'),
    ('map', 'freq', MAP, (2, 1, 7, 6, 6), (2, 1, 7), 'ijkl,ijlkn,ijnl->ijl'),
    ('map', 'pix', MAP, (2, 1, 6, 7, 7), (2, 1, 6), 'ijkl,ijkln,ijkn->ijk'),
]
CASE_IDS = ['%s-%s' % (c[0], c[1]) for c in CASES]
# the data axis the covariance couples, for the independent (O, n, I) recomputation of the host test
AXIS = {('vis', 'bl'): 2, ('vis', 'time'): 3, ('vis', 'freq'): 4, ('map', 'freq'): 2, ('map', 'pix'): 3}

# raw (O, n, I) problems of the GPU test: n in {1, 3, 17, 64, 65, 130, 257} x O in {1, 5} x I in {1, 3, 9} -- every
# lanes-per-row choice in both precisions (n = 12 and 24 are added for the 16-lane form, which the other sizes never reach
# under this planner), ragged row tails, rows of more than one 16-byte stride per lane, I = 1 / a ragged tile / more than
# one tile, one and several outer indices.  ONE pruning rule: a combination whose matrices O I n^2 exceed 600 000 complex
# numbers (4.8 MB in complex64, 9.6 MB in complex128) is left out, to keep every tensor at a few MB; that drops (5, 130, 9),
# (5, 257, 3) and (5, 257, 9).  (1, 257, 9), 594 441 numbers, runs in complex64 only (RAW_SHAPES_C64): the ragged second
# tile at the longest rows; in complex128 the same branch is reached by (1, 130, 9).
RAW_MAX_COMPLEX = 600000
_ALL = [(O, n, I) for n in (1, 3, 12, 17, 24, 64, 65, 130, 257) for O in (1, 5) for I in (1, 3, 9)]
RAW_SHAPES_C64 = [(1, 257, 9)]
RAW_SHAPES = [s for s in _ALL if s[0] * s[2] * s[1] ** 2 <= RAW_MAX_COMPLEX and s not in RAW_SHAPES_C64]
SPLIT_SHAPE = (2, 257, 1)                 # O I = 2 batches of 257 rows: the planner must split rows
CAPPED_SHAPE = (4500, 3, 2)               # more work-groups' worth of tiles than the 4096 blocks the launcher caps at
PLAN_N = sorted({n for _, n, _ in RAW_SHAPES} | {2048})


def hermitian_pd(rng, batch, n):
    """(batch..., n, n) complex128: A A^H + n I"""
    A = rng.normal(size=tuple(batch) + (n, n)) + 1j * rng.normal(size=tuple(batch) + (n, n))
    W = A @ np.conj(np.swapaxes(A, -1, -2)) + n * np.eye(n)
    return 0.5 * (W + np.conj(np.swapaxes(W, -1, -2)))


def cnormal(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


@functools.lru_cache(maxsize=None)
def public_problem(case, dtype, seed=0):
    """(pred, data, icov) of CASES[case] on the CPU in `dtype`; computed once, shared, not to be modified"""
    mode, axis, shape, icov_shape, _, _ = CASES[case]
    rng = np.random.default_rng(1000 * seed + case)
    W = hermitian_pd(rng, icov_shape[:-2], icov_shape[-1])
    return (torch.as_tensor(cnormal(rng, shape)).to(dtype), torch.as_tensor(cnormal(rng, shape)).to(dtype),
            torch.as_tensor(W).to(dtype))


def oracle_einsum(case, res, icov):
    """float64 per-batch res^H icov res of CASES[case] (real part; the imaginary one vanishes for Hermitian icov)"""
    r, W = res.to(torch.complex128), icov.to(torch.complex128)
    return torch.einsum(CASES[case][5], r.conj(), W, r).real


def oracle_loop(case, res, icov):
    """the same by a plain loop over batches: q[b] = r.conj() @ W[b] @ r with r the data along the covariance axis"""
    mode, cov_axis, shape, icov_shape, out_shape, _ = CASES[case]
    r = np.moveaxis(res.to(torch.complex128).numpy(), AXIS[(mode, cov_axis)], -1)       # batch axes in data order, then n
    W = icov.to(torch.complex128).numpy()
    out = np.zeros(out_shape)
    for b in np.ndindex(*out_shape):
        out[b] = (np.conj(r[b]) @ W[b] @ r[b]).real
    return torch.as_tensor(out)


@functools.lru_cache(maxsize=None)
def raw_problem(O, n, I, dtype, seed=0):
    """pred, data (O, n, I) and W (O, I, n, n) on the CPU in `dtype`, with the float64 references: y = W r (O, n, I),
    q (O, I), S (O, I) and Srow (O, n, I) of the bound.  Computed once per shape, shared, not to be modified."""
    rng = np.random.default_rng(seed + 7 * O + 131 * n + 1009 * I)
    pred = torch.as_tensor(cnormal(rng, (O, n, I))).to(dtype)
    data = torch.as_tensor(cnormal(rng, (O, n, I))).to(dtype)
    W = torch.as_tensor(hermitian_pd(rng, (O, I), n)).to(dtype)
    r = pred.to(torch.complex128) - data.to(torch.complex128)
    W64 = W.to(torch.complex128)
    y = torch.einsum('oiac,oci->oai', W64, r)
    q = (r.conj() * y).real.sum(1)
    Srow = torch.einsum('oiac,oci->oai', W64.abs(), r.abs())
    S = (r.abs() * Srow).sum(1)
    return dict(pred=pred, data=data, W=W, y=y, q=q, S=S, Srow=Srow)


def bound(n, dtype, S):
    """the bound C_ORDER (2 n + 8) u S of the module docstring, elementwise in S"""
    return C_ORDER * (2 * n + 8) * UNIT[dtype] * S
