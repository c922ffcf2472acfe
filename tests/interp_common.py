"""
Shared by tests/test_interp_host.py and tests/test_interp_gpu.py: a plain float64 numpy restatement of the operations of
csrc/interp.hip, written from their definitions, the error bound the GPU tests assert, and the deterministic case tables.

    gather          out[r, p]  = sum_k w[p, k] m[r, inds[p, k]]                      over the k with w[p, k] != 0
    gather_adjoint  gm[r, j]   = sum_{(p, k): inds[p, k] == j} w[p, k] gout[r, p]    over the same k
    beam_sky        psky[r, q] = gather(bmap)[r, q] sky[r, cut[q]],   0 where cut[q] == Npix
    beam_sky_grad_map, beam_sky_grad_sky: the two adjoints of beam_sky for a cotangent gpsky

Every function returns (value, S, n): S is the same sum with every factor replaced by its absolute value and n the number
of its terms, both per element (n broadcasts against value).  Complex maps are pairs of real ones (the weights are real), so
the real and the imaginary part are computed apart and S carries the bound of either in its own real / imaginary part.

ERROR BOUND.  The inputs are rounded to the working precision before these functions see them, so the only error of a
kernel is that of its arithmetic: fma chains (one rounding per term, whatever the order or the grouping into partial
sums), a few adds that join partial sums (the 4 entry slots of the CSR walk: 2; the time-split planes of the sky gradient:
at most 2 at the shapes used here) and one product (the sky factor of psky / of the transposed cotangent).  Each rounding
moves the result by at most u times the sum of absolute values, so an element is off by at most (n + 4) u S, with u = 2^-24
for float32 and 2^-53 for float64.  For the sky gradient n = (steps at which the pixel is visible) x (Nnn + 1): the Nnn
terms of each re-interpolated beam value and the product with the cotangent.  A dropped, doubled or misplaced term moves
an element by about S / n.
"""
import numpy as np

U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
RDT = {'f32': np.float32, 'f64': np.float64}
CDT = {'f32': np.complex64, 'f64': np.complex128}

# layout constants of csrc/interp.hip
RT = 8                                   # map rows per block of the gather
RB = 8                                   # rows per block of the row-major adjoint
GRID_Y = 65535                           # blocks along y of one launch
ROW_TILE = 64                            # rows (channels) per tile of the CSR scatter and of the psky builder
SCATTER_GRID_ROWS = 16 * ROW_TILE        # rows of one pass of the CSR scatter's row loop
SWEEP = 16                               # entries of one sweep of the CSR walk (4 slots x 4 deep)
GATHER_WIDTHS = (1, 4, 6, 9, 16)         # compile-time stencil widths of the gather; every other width is the generic one
PSKY_WIDTHS = (1, 4, 9, 16)              # ... of the psky builder and its sky gradient

PLANTED = (0, 1, 3, 4, 5, 15, 16, 17, 33, 100)     # list lengths every planted stencil holds


def bound(S, n, prec):
    return (np.asarray(n, dtype=np.float64) + 4.0) * U[prec] * S + 1e-300


def _parts(f, a, *rest):
    """f on the real and on the imaginary part of a complex first argument; the bounds travel as real / imaginary part of S"""
    if not np.iscomplexobj(a):
        return f(np.asarray(a, dtype=np.float64), *rest)
    (vr, sr, n), (vi, si, _) = f(a.real.astype(np.float64), *rest), f(a.imag.astype(np.float64), *rest)
    return vr + 1j * vi, sr + 1j * si, n


def _gather_real(m, inds, wgts):
    w = np.asarray(wgts, dtype=np.float64)
    live = w != 0
    with np.errstate(invalid='ignore'):
        near = m[:, inds]                                             # (R, P, Nnn)
        out = np.where(live, w * near, 0.0).sum(-1)
        S = np.where(live, np.abs(w) * np.abs(near), 0.0).sum(-1)
    return out, S, live.sum(-1)


def gather(m, inds, wgts):
    return _parts(_gather_real, m, inds, wgts)


def _adjoint_real(gout, inds, wgts, Npb):
    w = np.asarray(wgts, dtype=np.float64).reshape(-1)
    e = np.flatnonzero(w != 0)
    node, point = inds.reshape(-1)[e], e // inds.shape[1]
    gmT, ST = np.zeros((Npb, gout.shape[0])), np.zeros((Npb, gout.shape[0]))
    np.add.at(gmT, node, w[e, None] * gout.T[point])
    np.add.at(ST, node, np.abs(w[e, None]) * np.abs(gout.T[point]))
    return gmT.T.copy(), ST.T.copy(), np.bincount(node, minlength=Npb)


def gather_adjoint(gout, inds, wgts, Npb):
    return _parts(_adjoint_real, gout, inds, wgts, Npb)


def _cut_sky(sky, cut):
    """sky[r, cut[q]] with the zero column of the padding"""
    return np.concatenate([np.asarray(sky, dtype=np.float64), np.zeros((sky.shape[0], 1))], axis=1)[:, cut]


def beam_sky(bmap, sky, inds, wgts, cut):
    B, SB, n = _gather_real(np.asarray(bmap, dtype=np.float64), inds, wgts)
    ks = _cut_sky(sky, cut)
    return B * ks, SB * np.abs(ks), n + 1


def beam_sky_grad_map(gpsky, sky, inds, wgts, cut, Npb):
    T1 = np.asarray(gpsky, dtype=np.float64) * _cut_sky(sky, cut)
    gm, S, n = _adjoint_real(T1, inds, wgts, Npb)
    return gm, S, n + 1


def beam_sky_grad_sky(gpsky, bmap, inds, wgts, cut, Npix):
    B, SB, _ = _gather_real(np.asarray(bmap, dtype=np.float64), inds, wgts)
    q = np.flatnonzero(cut < Npix)
    g = np.asarray(gpsky, dtype=np.float64)
    gsT, ST = np.zeros((Npix, g.shape[0])), np.zeros((Npix, g.shape[0]))
    np.add.at(gsT, cut[q], (g * B).T[q])
    np.add.at(ST, cut[q], (np.abs(g) * SB).T[q])
    return gsT.T.copy(), ST.T.copy(), np.bincount(cut[q], minlength=Npix) * (inds.shape[1] + 1)


# ------------------------------------------------------------------------------------------------------- builders
def csr_lengths(inds, wgts, Npb):
    """list lengths of the inverse index, built the way ops.InterpStencil builds it: the entries of weight 0 stay out"""
    flat = inds.reshape(-1)
    keep = np.flatnonzero(wgts.reshape(-1) != 0)
    order = keep[np.argsort(flat[keep], kind='stable')]
    ptr = np.zeros(Npb + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(flat[keep], minlength=Npb))
    assert len(order) == ptr[-1]
    return np.diff(ptr)


def make_stencil(seed, Npb, P, Nnn, all_zero=False, dead_points=0, long=100):
    """
    (inds int64 (P, Nnn), wgts float64 (P, Nnn), planted): about 10 % of the weights are exactly 0 (at least one), the
    others +-[0.25, 1].  When the live entries suffice, the first nodes of a seeded permutation get lists of exactly the
    PLANTED lengths (the last one `long`) and `planted` maps length -> node; the other live entries are spread over the other
    nodes, the entries of weight 0 over ALL nodes (the node of the empty list included: they must not count).
    `dead_points`: that many points, listed in planted['dead'], have only weights 0.
    """
    rng = np.random.default_rng(seed)
    E = P * Nnn
    w = rng.uniform(0.25, 1.0, E) * rng.choice([-1.0, 1.0], E)
    dead = rng.choice(P, dead_points, replace=False) if dead_points else np.zeros(0, dtype=np.int64)
    w[rng.choice(E, max(1, int(round(0.1 * E))), replace=False)] = 0.0
    w.reshape(P, Nnn)[dead] = 0.0
    if all_zero:
        w[:] = 0.0
    live = np.flatnonzero(w != 0)
    lengths = PLANTED[:-1] + (long,)
    inds = rng.integers(0, Npb, E)
    planted = {'dead': dead}
    if len(live) >= sum(lengths) + 16 and Npb > len(lengths) + 1:
        nodes = rng.permutation(Npb)
        chosen, rest = nodes[:len(lengths)], nodes[len(lengths):]
        inds[live] = rng.choice(rest, len(live))
        take = rng.permutation(live)
        at = 0
        for L, j in zip(lengths, chosen):
            inds[take[at:at + L]] = j
            at += L
            planted[L] = int(j)
    return inds.reshape(P, Nnn), w.reshape(P, Nnn), planted


NEVER, ONCE, ALWAYS = 7, 8, 650          # sky pixels visible at no step, at step 0 alone, at every step


def make_cut(seed, Nt, Ps, Npix):
    """
    cut (Nt * Ps,) sky pixel of every point (Npix = padding) and pos (Nt, Npix) its inverse per step (-1 = not visible):
    ragged steps with padding, the last one full; with Nt > 2, step 1 sees the last 64-pixel tile alone; pixel NEVER (and
    the last of all) is visible at no step, ONCE at step 0 alone, ALWAYS at every step.
    """
    rng = np.random.default_rng(seed)
    last_tile = (Npix - 1) // 64 * 64
    assert last_tile <= ALWAYS < Npix - 1 and Ps <= last_tile - 3
    pool = np.setdiff1d(np.arange(last_tile), [NEVER, ONCE])
    cut = np.full((Nt, Ps), Npix, dtype=np.int64)
    pos = np.full((Nt, Npix), -1, dtype=np.int64)
    for t in range(Nt):
        if Nt > 2 and t == 1:
            c = np.arange(last_tile, Npix - 1)
        else:
            n = Ps if t == Nt - 1 else int(rng.integers(100, Ps - 1))
            c = np.concatenate([rng.choice(pool, n - 1 - (t == 0), replace=False), [ALWAYS], [ONCE] if t == 0 else []])
            c = np.sort(c.astype(np.int64))
        cut[t, :len(c)] = c
        pos[t, c] = np.arange(len(c))
    return cut.reshape(-1), pos


def sky_grad_splits(R, Npix, Nt):
    """time splits of the sky gradient and steps per split: enough blocks for 8 per CU, at least 4 steps per split"""
    blocks = ((Npix + 63) // 64) * ((R + 63) // 64)
    S = max(1, min((Nt + 3) // 4, (2048 + blocks - 1) // blocks, 64))
    Tc = (Nt + S - 1) // S
    return (Nt + Tc - 1) // Tc, Tc


# ------------------------------------------------------------------------------------------------------- case tables
# 1. gather forward + adjoint across the widths: (Nnn, cplx, prec, R, P, padded)
GATHER_NNN = (1, 2, 3, 4, 6, 8, 9, 12, 16)
GATHER_R = (1, 7, 8, 9, 17)
GATHER_P = (1, 255, 256, 257)
GATHER_NPB = 41
GATHER_CASES = [(Nnn, cplx, prec, GATHER_R[(i + j) % 5], GATHER_P[(i + 2 * j + 1) % 4], bool((i + (j >> 1)) % 2))
                for i, Nnn in enumerate(GATHER_NNN)
                for j, (cplx, prec) in enumerate([(False, 'f32'), (True, 'f64'), (True, 'f32'), (False, 'f64')])]

# 2. weights 0 against non-finite entries: (Nnn, cplx, prec)
POISON_NNN = (1, 4, 8, 12)
POISON_CASES = [(Nnn, cplx, prec) for Nnn in POISON_NNN for cplx, prec in [(False, 'f32'), (True, 'f64')]]
POISON_R, POISON_P = 9, 257

# 3. CSR scatter: (Nnn, R, cplx, prec); RN = R (2 R when complex)
SCATTER_NPB, SCATTER_P = 37, 300
SCATTER_NNN = (4, 16, 6, 9)
SCATTER_ROWS = ((4, False), (6, False), (64, False), (68, False), (1028, False), (515, True))
SCATTER_CASES = [(Nnn, R, cplx, prec) for Nnn in SCATTER_NNN for R, cplx in SCATTER_ROWS for prec in ('f32', 'f64')]

# 4. row-major scatter of the one-node stencil: (R, cplx, prec, Npb, extra stride)
ROWS_P = 600
ROWS_R = (1, 7, 8, 9, 23)
ROWS_NPB = (255, 256, 257)
ROWS_CASES = [(R, cplx, prec, ROWS_NPB[(i + 2 * c + p) % 3], 37 * ((i + c + p) % 2))
              for i, R in enumerate(ROWS_R) for c, cplx in enumerate((False, True)) for p, prec in enumerate(('f32', 'f64'))]

# 5. rows beyond one grid
BIG_R, BIG_NPB, BIG_P = GRID_Y * RT + 9, 3, 5

# 6. psky builder: (Nnn, prec, R, Nt).  Nt = 3: no time split; 6 and 9: whole splits (2 x 3, 3 x 3); 7: a ragged last one (4 + 3)
PSKY_NPB, PSKY_NPIX, PSKY_PS = 257, 700, 256
PSKY_NNN = (1, 2, 4, 8, 9, 16)
PSKY_R = (37, 66, 72)
PSKY_NT = (3, 6, 7, 9)
PSKY_CASES = [(Nnn, prec, R, Nt) for Nnn in PSKY_NNN for prec in ('f32', 'f64') for R in PSKY_R for Nt in PSKY_NT]


def stencil_seed(*key):
    return int(np.random.SeedSequence([abs(int(k)) for k in key]).generate_state(1)[0])
