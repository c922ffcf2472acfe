"""
Shared by tests/test_coupling_host.py, tests/test_coupling_gpu.py and tests/golden/make_golden_coupling.py: a float64 numpy
restatement of the mutual-coupling term (table building, forward, both gradients), written from the formulas of
include/rime_hip.h and of the reference module, the case tables, and the derived accuracy bound.

Formulas.  With V the N x N matrix read from the data through the table (row, conjugated row, or zero), Xd = X o D,
E = [I] + Xd (double: + Xd Xd), G the cotangent placed at the output entries of the matrix (zero elsewhere):
    W  = E V E^H            ('left': E V,  'right': V E^H)
    gV = E^H G E            ('left': E^H G,  'right': G E);   gdata[row] = sum of gV at the entries that read the row
                            unconjugated and of conj(gV) at those that read it conjugated
    gE = G E V^H + G^H E V  ('left': G V^H,  'right': G^H V);  double: gXd = gE + gE Xd^H + Xd^H gE, else gXd = gE
    gX = gXd o conj(D), summed over t when X has one time and over f when it has one channel
Cotangents follow torch's convention for complex tensors (the gradient of a real loss with respect to conj(z), times two).

The bound (derived, not measured; fixed by the design of the kernel, not by its results).  u = 2^-24 or 2^-53,
gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  A complex dot product of
length N accumulated with FMAs rounds 2 N times per real component, and a real component of sum a_k b_k and of its error are
bounded through the moduli, sum |a_k| |b_k|.  Per real component of every output element
    |error| <= sqrt(2) gamma_n(u) M
where M is the SAME formula evaluated on the moduli |X|, |D|, |data|, |G| (so M = (|E|~ |V| |E|~^T)[a, b] for the forward,
with |E|~ = [I] + |X| |D| (+ |Xd| |Xd|) >= |E| entrywise: forming E rounds too, and a diagonal that cancels must not shrink the
bound), the factor sqrt(2) turns the componentwise error of an intermediate into the modulus the next product sees, and n
counts the roundings on the longest path to the element:
    nE       E as an operand: Xd = X o D 2, + I 1 -> 3;  double: two operands Xd 4, the dot 2 N, the addend Xd + I 3, the add 1
             -> 2 N + 8
    forward  'both' 2 nE + 4 N (T = E V, then T E^H);  'left' / 'right' nE + 2 N
    gdata    'both' P = G E (nE + 2 N), then P^H E + E^H P as ONE chain of 4 N with E again: 2 nE + 6 N;  else nE + 4 N
    gX       'both' P and T = E V carry nE + 2 N each, P V^H + G^H T is one chain of 4 N: nE + 6 N;  else 2 N;  then
             o conj(D) 2;  double: gE of the dense E as above, then the chain 4 N, its operands Xd 2, the addend 1: + 4 N + 3;
             the broadcast sums add Nt Nf - 1, Nt - 1 or Nf - 1
These are upper counts for every variant (without dly or identity there are fewer roundings).  The restatement runs in
float64 with numpy's own summation order, so a comparison counts both: gamma_n(u_kernel) + gamma_n(2^-53).  Against the
reference-generated fixture (float64, another order again) the same bound is used with u = 2^-53 and both orders counted;
where the cotangent is itself computed from the output (the fixture's loss sum w |W|^2) its moduli are taken from the bound
of the forward and its roundings (the forward's n + 2) are added.  Where the module under test evaluates the delay phasor
itself, its D differs from the recorded one by dly_ulps(...) u per component (two evaluations of a phase of up to ~100 rad);
that relative perturbation of an input is propagated like roundings at every place D enters (roundings(..., dly=)).
The tests assert error / bound <= 1 for every component and print the worst ratio.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
CONJ = 1 << 30
TILE = 32                      # matrix tile of the kernel (csrc/coupling.hip, CP_TILE); the case table straddles it
NT, NF = 3, 5                  # the fixture
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(HERE, 'golden', 'coupling.npz')) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


# fixture cases: tag -> keywords (tb: params with one time bin, broadcast)
GOLDEN_CASES = {}
for _prod in ('both', 'left', 'right'):
    for _addI in (True, False):
        for _double in (False, True):
            for _tb in (False, True):
                GOLDEN_CASES['%s_%s_%s_%s' % (_prod, 'I' if _addI else 'noI', 'dbl' if _double else 'sgl', 'tb' if _tb else 'pt')] = \
                    dict(prod=_prod, add_I=_addI, double=_double, tb=_tb)

# kernel cases: N straddles the matrix tile (1, 3, 8, tile - 1, tile, tile + 1, 65: three tiles with a ragged last one), Nf the
# channel run of 8 (1, 5, 37), Nt 1 and 3; Tm / Fm: does the coupling have the time / channel axis; layout 'full' (every
# ant2 >= ant1 pair), 'nulls' (cross baselines and autos missing), 'noautos'; antenna numbers are never in ascending order
KERNEL_CASES = {
    'n1': dict(N=1, Nt=1, Nf=1, Tm=True, Fm=True, dly=True, prod='both', add_I=True, double=False, layout='full'),
    'n3_left': dict(N=3, Nt=3, Nf=5, Tm=True, Fm=True, dly=True, prod='left', add_I=True, double=False, layout='nulls'),
    'n3_right': dict(N=3, Nt=3, Nf=5, Tm=False, Fm=True, dly=True, prod='right', add_I=False, double=False, layout='nulls'),
    'n8_both': dict(N=8, Nt=3, Nf=5, Tm=True, Fm=True, dly=True, prod='both', add_I=True, double=False, layout='nulls'),
    'n8_tb': dict(N=8, Nt=3, Nf=5, Tm=False, Fm=True, dly=True, prod='both', add_I=True, double=False, layout='noautos'),
    'n8_fb': dict(N=8, Nt=3, Nf=37, Tm=True, Fm=False, dly=True, prod='both', add_I=True, double=False, layout='nulls'),
    'n8_tfb': dict(N=8, Nt=3, Nf=5, Tm=False, Fm=False, dly=True, prod='both', add_I=False, double=False, layout='full'),
    'n8_nodly': dict(N=8, Nt=1, Nf=37, Tm=True, Fm=True, dly=False, prod='both', add_I=True, double=False, layout='nulls'),
    'n8_dbl': dict(N=8, Nt=3, Nf=5, Tm=True, Fm=True, dly=True, prod='both', add_I=True, double=True, layout='nulls'),
    'n8_dbl_tb': dict(N=8, Nt=3, Nf=5, Tm=False, Fm=True, dly=True, prod='left', add_I=False, double=True, layout='nulls'),
    'n8_dbl_fb': dict(N=8, Nt=1, Nf=5, Tm=True, Fm=False, dly=True, prod='right', add_I=True, double=True, layout='full'),
    'n8_dbl_nodly': dict(N=8, Nt=3, Nf=1, Tm=False, Fm=True, dly=False, prod='both', add_I=True, double=True, layout='noautos'),
    'n31': dict(N=31, Nt=1, Nf=5, Tm=True, Fm=True, dly=True, prod='both', add_I=True, double=False, layout='nulls'),
    'n32': dict(N=32, Nt=1, Nf=5, Tm=True, Fm=True, dly=True, prod='right', add_I=True, double=False, layout='full'),
    'n33': dict(N=33, Nt=3, Nf=5, Tm=False, Fm=True, dly=True, prod='both', add_I=True, double=False, layout='nulls'),
    'n33_left': dict(N=33, Nt=1, Nf=37, Tm=True, Fm=True, dly=True, prod='left', add_I=False, double=False, layout='noautos'),
    'n33_dbl': dict(N=33, Nt=1, Nf=5, Tm=True, Fm=True, dly=True, prod='both', add_I=True, double=True, layout='nulls'),
    'n65': dict(N=65, Nt=3, Nf=37, Tm=False, Fm=True, dly=True, prod='both', add_I=True, double=False, layout='nulls'),
    'n65_pt': dict(N=65, Nt=3, Nf=5, Tm=True, Fm=True, dly=True, prod='both', add_I=True, double=False, layout='noautos'),
    'n65_right': dict(N=65, Nt=1, Nf=1, Tm=True, Fm=True, dly=False, prod='right', add_I=True, double=False, layout='nulls'),
}


def build_table(ants, bls):
    """(table [N, N], out_rows [Nbl]) of antennas `ants` (the matrix order) and baselines `bls`, with the loops of the
    reference's setup_coupling: entry (i, j) looks (ant_i, ant_j) up when ant_j >= ant_i, else (ant_j, ant_i) conjugated"""
    N = len(ants)
    table = np.full((N, N), -1, dtype=np.int64)
    bls = [tuple(int(x) for x in b) for b in bls]
    for i, a1 in enumerate(ants):
        for j, a2 in enumerate(ants):
            if a2 >= a1:
                if (a1, a2) in bls:
                    table[i, j] = bls.index((a1, a2))
            elif (a2, a1) in bls:
                table[i, j] = bls.index((a2, a1)) | CONJ
    ants = list(ants)
    out_rows = np.array([ants.index(b[0]) * N + ants.index(b[1]) for b in bls], dtype=np.int64)
    return table, out_rows


def _mm(A, B):
    return np.einsum('iktf,kjtf->ijtf', A, B)


def _H(A):
    return np.conj(A).transpose(1, 0, 2, 3)


def _matrix(rows, table, Nt, Nf):
    N = table.shape[0]
    V = np.zeros((N, N, Nt, Nf), dtype=np.complex128)
    for a in range(N):
        for b in range(N):
            e = int(table[a, b])
            if e >= 0:
                V[a, b] = np.conj(rows[e & (CONJ - 1)]) if e & CONJ else rows[e]
    return V


def _build_E(X, D, add_I, double, Nt, Nf):
    N = X.shape[0]
    Xd = np.broadcast_to(X * D if D is not None else X, (N, N, Nt, Nf)).astype(np.complex128)
    E = Xd + _mm(Xd, Xd) if double else Xd.copy()
    if add_I:
        E = E + np.eye(N)[:, :, None, None]
    return Xd, E


def evaluate(X, D, data, table, out_rows, add_I, prod, double, G=None):
    """X (N, N, Tm, Fm), D (N, N, 1, Nf) or None, data (Nbl, Nt, Nf), G (Nout, Nt, Nf) or None -> (W rows, gdata, gX); called
    with the moduli of every input it returns the M of the bound"""
    Nbl, Nt, Nf = data.shape
    N = table.shape[0]
    Xd, E = _build_E(X, D, add_I, double, Nt, Nf)
    V = _matrix(data, table, Nt, Nf)
    W = {'both': lambda: _mm(_mm(E, V), _H(E)), 'left': lambda: _mm(E, V), 'right': lambda: _mm(V, _H(E))}[prod]()
    rows = W.reshape(N * N, Nt, Nf)[out_rows]
    if G is None:
        return rows, None, None
    Gm = np.zeros((N * N, Nt, Nf), dtype=np.complex128)
    Gm[out_rows] = G
    Gm = Gm.reshape(N, N, Nt, Nf)
    if prod == 'both':
        gV, gE = _mm(_mm(_H(E), Gm), E), _mm(_mm(Gm, E), _H(V)) + _mm(_mm(_H(Gm), E), V)
    elif prod == 'left':
        gV, gE = _mm(_H(E), Gm), _mm(Gm, _H(V))
    else:
        gV, gE = _mm(Gm, E), _mm(_H(Gm), V)
    gdata = np.zeros((Nbl, Nt, Nf), dtype=np.complex128)
    for a in range(N):
        for b in range(N):
            e = int(table[a, b])
            if e >= 0:
                gdata[e & (CONJ - 1)] += np.conj(gV[a, b]) if e & CONJ else gV[a, b]
    gXd = gE + _mm(gE, _H(Xd)) + _mm(_H(Xd), gE) if double else gE
    gX = gXd * np.conj(D) if D is not None else gXd
    if X.shape[2] == 1 and Nt > 1:
        gX = gX.sum(axis=2, keepdims=True)
    if X.shape[3] == 1 and Nf > 1:
        gX = gX.sum(axis=3, keepdims=True)
    return rows, gdata, gX


def magnitudes(X, D, data, table, out_rows, add_I, prod, double, G=None):
    """the M of the bound: evaluate() on the moduli"""
    ab = lambda a: None if a is None else np.abs(a).astype(np.complex128)
    return tuple(None if m is None else m.real for m in evaluate(ab(X), ab(D), ab(data), table, out_rows, add_I, prod, double, ab(G)))


def dly_ulps(freqs, antvecs, k=10):
    """m such that two float64 evaluations of the delay phasor exp(i phi), phi = 2 pi (f - f0) / c * |r_j - r_i|, differ by at
    most m 2^-53 per component: each evaluates phi with at most k = 10 roundings (f - f0, pi, two products, the quotient, and
    for the length three differences, three squares, two sums and the root, each entering phi to first order at most once), so
    |delta phi| <= 2 k u max|phi|, which moves a point of the unit circle by as much; sine and cosine are within one ulp of a
    value <= 1 on either side: + 2"""
    fr, v = np.asarray(freqs, dtype=np.float64), np.asarray(antvecs, dtype=np.float64)
    L = np.linalg.norm(v[:, None] - v[None], axis=-1).max()
    return 2 * k * 2 * np.pi * (fr.max() - fr[0]) / 2.99792458e8 * L + 2


def roundings(N, Nt, Nf, Tm, Fm, prod, double, dly=0):
    """(n forward, n gdata, n gX) as counted in the module docstring; Tm, Fm: the extents of X; dly: a relative perturbation
    of D of `dly` units of u (two evaluations of the phasor, dly_ulps) counts as that many roundings wherever D enters: once
    in Xd, so once per E (twice for the double path, where |Xd| |Xd| is part of |E|~), and once more in gX = gXd o conj(D)"""
    nE = (2 * N + 8 if double else 3) + (2 * dly if double else dly)
    two = prod == 'both'
    nf = 2 * nE + 4 * N if two else nE + 2 * N
    nd = 2 * nE + 6 * N if two else nE + 4 * N
    nx = (nE + 6 * N if two else 2 * N) + 2 + dly + (4 * N + 3 + dly if double else 0)
    nx += (Nt if Tm == 1 else 1) * (Nf if Fm == 1 else 1) - 1
    return nf, nd, nx


def gamma(n, u):
    return n * u / (1 - n * u)


def bound(M, n, prec, orders=1):
    """sqrt(2) (orders * gamma_n(u) + gamma_n(2^-53)) M: the kernel in `prec` (counted `orders` times: the fixture was summed
    in another order than either side) against a float64 restatement"""
    return np.sqrt(2.0) * (orders * gamma(n, U[prec]) + gamma(n, U['f64'])) * M


def ratio(got, want, bnd):
    """worst |got - want| / bound over the real components; a zero bound demands equality (ratio 0 or inf)"""
    worst = 0.0
    for part in ('real', 'imag'):
        e = np.abs(getattr(got, part).astype(np.float64) - getattr(want, part))
        r = np.where(bnd > 0, e / np.where(bnd > 0, bnd, 1), np.where(e == 0, 0.0, np.inf))
        worst = max(worst, float(r.max()))
    return worst


def array_layout(N, layout, seed):
    """(ants in matrix order -- never ascending for N > 1 --, bls): every ant2 >= ant1 pair ('full'), minus every fifth cross
    baseline and every third auto ('nulls'), or minus all autos ('noautos')"""
    rng = np.random.default_rng(seed)
    ants = [int(a) for a in rng.permutation(N) * 3 + 1]
    if N > 1 and ants == sorted(ants):
        ants = ants[::-1]
    pairs = [(a, b) for a in sorted(ants) for b in sorted(ants) if b >= a]
    if layout == 'nulls' and N > 1:
        cross = [p for p in pairs if p[0] != p[1]]
        autos = [p for p in pairs if p[0] == p[1]]
        pairs = [p for k, p in enumerate(cross) if k % 5 != 2] + [p for k, p in enumerate(autos) if k % 3 != 1]
    elif layout == 'noautos' and N > 1:
        pairs = [p for p in pairs if p[0] != p[1]]
    order = rng.permutation(len(pairs))
    return ants, [pairs[k] for k in order]


def case_inputs(name, seed=0):
    """float32-exact complex128 inputs of a kernel case: dict(X, D, data, G, table, out_rows) + the case keywords"""
    c = dict(KERNEL_CASES[name])
    rng = np.random.default_rng([seed, sorted(KERNEL_CASES).index(name)])
    N, Nt, Nf = c['N'], c['Nt'], c['Nf']
    ants, bls = array_layout(N, c['layout'], seed + N)
    table, out_rows = build_table(ants, bls)

    def cx(*shape, scale=1.0):
        z = (rng.normal(size=shape) + 1j * rng.normal(size=shape)) * scale
        return z.astype(np.complex64).astype(np.complex128)

    c['X'] = cx(N, N, Nt if c['Tm'] else 1, Nf if c['Fm'] else 1, scale=0.3)
    ph = rng.uniform(0, 2 * np.pi, size=(N, N, 1, Nf))
    c['D'] = np.exp(1j * ph).astype(np.complex64).astype(np.complex128) if c['dly'] else None
    c['data'] = cx(len(bls), Nt, Nf)
    c['G'] = cx(len(bls), Nt, Nf)
    c['table'], c['out_rows'], c['ants'], c['bls'] = table, out_rows, ants, bls
    return c


def golden_inputs(tag):
    g = golden()
    kw = GOLDEN_CASES[tag]
    p = g['p_tb' if kw['tb'] else 'p_pt']
    X = (p[..., 0] + 1j * p[..., 1])[0, 0]
    table, out_rows = build_table([int(a) for a in g['ants']], g['bls'])
    return kw, X, g['dly_ct'][0, 0], g['data'][0, 0], g['w'][0, 0], table, out_rows


def golden_bounds(tag, own_dly=False):
    """(W, gdata, gX, their bounds) of the restatement for a recorded case; the cotangent 2 w W comes from the output, so its
    moduli are those of the forward bound and its roundings are added.  own_dly: the side under test evaluates the delay
    phasor itself instead of taking the recorded one; the bound then covers that difference of the inputs (dly_ulps)"""
    kw, X, D, data, w, table, out_rows = golden_inputs(tag)
    args = (table, out_rows, kw['add_I'], kw['prod'], kw['double'])
    W, _, _ = evaluate(X, D, data, *args)
    G = 2 * w * W
    _, gd, gx = evaluate(X, D, data, *args, G=G)
    Mw, _, _ = magnitudes(X, D, data, *args)
    _, Md, Mx = magnitudes(X, D, data, *args, G=2 * w * Mw)
    N, (Nbl, Nt, Nf) = X.shape[0], data.shape
    m = dly_ulps(golden()['freqs'], golden()['antvecs']) / 2 if own_dly else 0      # bound() counts n once per side
    nf, nd, nx = roundings(N, Nt, Nf, X.shape[2], X.shape[3], kw['prod'], kw['double'], dly=m)
    return (W, gd, gx), (bound(Mw, nf, 'f64'), bound(Md, nd + nf + 2, 'f64'), bound(Mx, nx + nf + 2, 'f64'))
