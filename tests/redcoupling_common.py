"""
Shared by tests/test_redcoupling_host.py, tests/test_redcoupling_gpu.py and tests/golden/make_golden_redcoupling.py: a float64
numpy restatement of the redundant-coupling term (entry list, the three orderings and their segments, the forward and both
gradients), written from the entry formula and not from the kernel, the case tables, and the derived accuracy bound.

Formulas.  Entry e = (row i, column j, conj flag, a, b), C = X o D:
    coef(e)  = (a >= 0 ? C[a] : 1) (b >= 0 ? conj(C[b]) : 1),      v(e) = conj(data[j]) if flag else data[j]
    out[i]   = sum over the entries of row i of coef v
    gdata[j] = sum over the entries of column j of  conj(coef) G[i]  (flag 0)  or  coef conj(G[i])  (flag 1)
    gC[c]    = sum over the entries with a == c of conj(conj(C[b]) v) G[i]  +  over those with b == c of (C[a] v) conj(G[i])
    gX       = gC o conj(D), summed over t when X has one time and over f when it has one channel
Cotangents follow torch's convention for complex tensors.

The bound (derived, not measured; fixed by the design of the kernel, not by its results).  u = 2^-24 or 2^-53,
gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  Per real component
    |error| <= sqrt(2) gamma_n(u) M
with M the same sum over the moduli |X|, |D|, |data|, |G| (evaluate() on the absolute values) and n the roundings on the
longest chain to an element.  A complex product by FMAs rounds twice per real component, a complex multiply-add onto an
accumulator twice as well:
    C = X o D 2, for a and for b: 4;  coef = C[a] conj(C[b]) 2;  so a coefficient carries at most 6
    forward  6 + 2 L_row,  L_row the longest row list
    gdata    6 + 2 L_col,  L_col the longest column list
    gX       w = conj(C[b]) v or C[a] v: 2 + 2;  the chain of a segment 2 min(SEG, L_term);  o conj(D) 2;  the combine: a wave
             adds ceil(nseg / WAVES) segment sums, each over Nt times when Tm = 1 and over ceil(Nf / COLS) channels of its lane
             when Fm = 1: that many additions, the butterfly log2(COLS) = 6 more when Fm = 1, the wave sums WAVES - 1
The restatement sums in numpy's own order (np.add.at, entry order) over the whole list, so its own count takes the full
list length L in place of the segment and the combine, plus the broadcast sums; a comparison counts both sides,
gamma_n(u_kernel) + gamma_n'(2^-53).  Against the reference-generated fixture (float64, another order again: dense matrices
and einsum over all Nin columns) the restatement's count is used for both sides with u = 2^-53; where the cotangent is computed
from the output (the fixture's loss sum w |Vc|^2) its moduli come from the forward bound's M and the forward's roundings + 2
are added; a delay phasor evaluated by the side under test differs from the recorded one by dly_ulps(...) u per component
(coupling_common.dly_ulps, the same two evaluations of a phase), counted wherever D enters: once per C (up to twice per
coefficient) and once more in gX.  The tests assert error / bound <= 1 for every component and print the worst ratio.
"""
import os

import numpy as np

import coupling_common as cc

HERE = os.path.dirname(os.path.abspath(__file__))
U = cc.U
FLAG = 1 << 30
SEG, WAVES, COLS = 64, 4, 64               # csrc/redcoupling.hip: ops.REDCOUPLING_SEG, RC_WAVES, RC_COLS
NT, NF = 3, 5                              # the fixture
TUPLES = ('unconj_param_unconj_vis', 'unconj_param_conj_vis', 'conj_param_unconj_vis', 'conj_param_conj_vis',
          'sq_param_unconj_vis', 'sq_param_conj_vis')
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(HERE, 'golden', 'redcoupling.npz')) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


# fixture cases: a covering table of use_reds x compress_to_red x include_second_order x time axis (tb: one time bin), every
# value of every keyword occurs; 'cuts' has max_len / second_max_len cuts and no_auto_coupling terms, so that names of Arows
# have no index in coupling_idx; min_dly is set where given
GOLDEN_CASES = {
    'red_cmp_sq_pt': dict(use_reds=True, compress=True, second=True, tb=False),
    'red_all_fo_tb': dict(use_reds=True, compress=False, second=False, tb=True),
    'phys_cmp_fo_pt': dict(use_reds=False, compress=True, second=False, tb=False, min_dly=20.0),
    'phys_all_sq_tb': dict(use_reds=False, compress=False, second=True, tb=True),
    'cuts': dict(use_reds=True, compress=True, second=True, tb=True, no_auto=True, term_max_len=31.0,
                 setup=dict(max_len=16.0, second_max_len=15.0), min_dly=20.0),
}


def entries(tuples, Nout, red_bl_inds=None):
    """the entry arrays (row, col, conj, a, b) of the six index tuples, in the order forward adds them up: zeroth order
    (column red_bl_inds[i], or i), then per kind of visibility the first-order terms and the second-order products; a kind
    without a first-order term is skipped entirely, as the reference skips its matrix"""
    ent = [(i, int(red_bl_inds[i]) if red_bl_inds is not None else i, 0, -1, -1) for i in range(Nout)]
    T = {k: [np.asarray(x).astype(np.int64) for x in tuples[k]] for k in TUPLES}
    for cv, kind in enumerate(('unconj_vis', 'conj_vis')):
        un, co, sq = T['unconj_param_' + kind], T['conj_param_' + kind], T['sq_param_' + kind]
        if len(un[0]) == 0 and len(co[0]) == 0:
            continue
        ent += [(i, j, cv, c, -1) for i, j, c in zip(*un)]
        ent += [(i, j, cv, -1, c) for i, j, c in zip(*co)]
        ent += [(sq[0][k], sq[1][k], cv, c1, c2) for k, c1, c2 in zip(sq[2], sq[3], sq[4])]
    return tuple(np.array([e[n] for e in ent], dtype=np.int64) for n in range(5))


def build_plan(row, col, conj, a, b, Nout, Nin, Nterms, seg=SEG):
    """the tables of ops.RedCouplingPlan with explicit loops: entries sorted by row (stable), and the orderings"""
    order = sorted(range(len(row)), key=lambda e: row[e])
    row, col, conj, a, b = ([int(x[e]) for e in order] for x in (row, col, conj, a, b))
    P = dict(ent=np.array([[row[e], col[e] | (FLAG if conj[e] else 0), a[e], b[e]] for e in range(len(row))], dtype=np.int32))
    byrow, bycol, byterm = [[] for _ in range(Nout)], [[] for _ in range(Nin)], [[] for _ in range(Nterms)]
    for e in range(len(row)):
        byrow[row[e]].append(e)
        bycol[col[e]].append(e)
        if a[e] >= 0:
            byterm[a[e]].append(e)
        if b[e] >= 0:
            byterm[b[e]].append(e | FLAG)
    csr = lambda lists: np.cumsum([0] + [len(x) for x in lists]).astype(np.int32)
    flat = lambda lists: np.array([x for lst in lists for x in lst], dtype=np.int32)
    P.update(roff=csr(byrow), coff=csr(bycol), cmem=flat(bycol), toff=csr(byterm), tmem=flat(byterm))
    assert (flat(byrow) == np.arange(len(row))).all()
    segterm, segstart, tsoff = [], [], [0]
    for c, lst in enumerate(byterm):
        for s in range(0, len(lst), seg):
            segterm.append(c)
            segstart.append(int(P['toff'][c]) + s)
        tsoff.append(len(segterm))
    P.update(segterm=np.array(segterm, dtype=np.int32), segstart=np.array(segstart, dtype=np.int32), tsoff=np.array(tsoff, dtype=np.int32))
    P.update(Lrow=max(map(len, byrow)), Lcol=max(map(len, bycol)), Lterm=max(map(len, byterm)), Nent=len(row),
             term_counts=np.array([len(x) for x in byterm]))
    return P


def evaluate(X, D, data, ent, Nout, G=None):
    """X (Nterms, Tm, Fm), D (Nterms, Nf) or None, data (Nin, Nt, Nf), ent = (row, col, conj, a, b), G (Nout, Nt, Nf) or None
    -> (out, gdata, gX); called with the moduli of every input it returns the M of the bound"""
    row, col, conj, a, b = ent
    Nin, Nt, Nf = data.shape
    Nterms = X.shape[0]
    C = np.broadcast_to(X * D[:, None, :] if D is not None else X, (Nterms, Nt, Nf)).astype(np.complex128)
    one = np.ones((1, Nt, Nf), dtype=np.complex128)
    Ca = np.where((a >= 0)[:, None, None], C[np.maximum(a, 0)], one)
    Cb = np.where((b >= 0)[:, None, None], np.conj(C[np.maximum(b, 0)]), one)
    v = np.where((conj > 0)[:, None, None], np.conj(data[col]), data[col])
    out = np.zeros((Nout, Nt, Nf), dtype=np.complex128)
    np.add.at(out, row, Ca * Cb * v)
    if G is None:
        return out, None, None
    g = G[row]
    gdata = np.zeros((Nin, Nt, Nf), dtype=np.complex128)
    np.add.at(gdata, col, np.where((conj > 0)[:, None, None], Ca * Cb * np.conj(g), np.conj(Ca * Cb) * g))
    gC = np.zeros((Nterms, Nt, Nf), dtype=np.complex128)
    np.add.at(gC, a[a >= 0], (np.conj(Cb * v) * g)[a >= 0])
    np.add.at(gC, b[b >= 0], (Ca * v * np.conj(g))[b >= 0])
    gX = gC * np.conj(D[:, None, :]) if D is not None else gC
    if X.shape[1] == 1 and Nt > 1:
        gX = gX.sum(axis=1, keepdims=True)
    if X.shape[2] == 1 and Nf > 1:
        gX = gX.sum(axis=2, keepdims=True)
    return out, gdata, gX


def magnitudes(X, D, data, ent, Nout, G=None):
    ab = lambda x: None if x is None else np.abs(x).astype(np.complex128)
    return tuple(None if m is None else m.real for m in evaluate(ab(X), ab(D), ab(data), ent, Nout, ab(G)))


def roundings(P, Nt, Nf, Tm, Fm, dly=0):
    """((n forward, n gdata, n gX) of the kernel, the same of the numpy restatement) as counted in the module docstring;
    dly: a relative perturbation of D in units of u, counted where D enters"""
    bt, bf = (Nt if Tm == 1 else 1), (Nf if Fm == 1 else 1)
    nseg = -(-P['Lterm'] // SEG)
    comb = -(-nseg // WAVES) * bt * (-(-Nf // COLS) if Fm == 1 else 1) + (6 if Fm == 1 else 0) + WAVES - 1
    kern = (6 + 2 * P['Lrow'] + 2 * dly, 6 + 2 * P['Lcol'] + 2 * dly, 4 + 2 * min(SEG, P['Lterm']) + 2 + comb + 2 * dly)
    ref = (6 + 2 * P['Lrow'] + 2 * dly, 6 + 2 * P['Lcol'] + 2 * dly, 6 + 2 * P['Lterm'] + bt * bf + 2 * dly)
    return kern, ref


def bound(M, n_kernel, prec, n_ref):
    return np.sqrt(2.0) * (cc.gamma(n_kernel, U[prec]) + cc.gamma(n_ref, U['f64'])) * M


ratio = cc.ratio


# ---- arrays -----------------------------------------------------------------------------------------------------------
def hex_positions(n, outrigger=False, shuffle=True, D=14.6):
    """(ants, (Nant, 3) positions) of a hexagon with n antennas on a side, optionally plus one outrigger, in an antenna order
    that is not ascending"""
    xs, ys = [], []
    for r in range(2 * n - 1):
        m = n + (r if r < n else 2 * n - 2 - r)
        for j in range(m):
            xs.append((-0.5 * (m - n) + j) * D)
            ys.append(r * np.sin(np.pi / 3) * D)
    vecs = np.stack([xs, ys, np.zeros(len(xs))], axis=1)
    vecs -= vecs.mean(axis=0)
    ants = list(range(len(xs)))
    if outrigger:
        ants.append(len(ants) + 3)
        vecs = np.concatenate([vecs, [[60.0, -25.0, 0.5]]])
    if shuffle and len(ants) > 2:
        order = np.random.default_rng(len(ants)).permutation(len(ants))
        ants, vecs = [ants[k] for k in order], vecs[order]
        assert ants != sorted(ants)
    return ants, vecs


def array_bls(ants, vecs, autos=True, redtol=1.0):
    """(bls_out: every ant2 >= ant1 pair, autos first if asked; bls_red: the first baseline of every redundant group)"""
    s = sorted(ants)
    pos = {a: v for a, v in zip(ants, vecs)}
    bls = ([(a, a) for a in s] if autos else []) + [(a, b) for a in s for b in s if b > a]
    reds, rv = [], []
    for bl in bls:
        v = pos[bl[1]] - pos[bl[0]]
        for k, r in enumerate(rv):
            if np.linalg.norm(r - v) < redtol:
                break
        else:
            rv.append(v)
            reds.append(bl)
    return bls, reds


# kernel cases.  array: (hexagon side, outrigger) or 'pair' (two antennas, one baseline); Nf 1, 5, 70 (crosses one wave of
# columns together with Nt); Tm / Fm: does the coupling have the time / channel axis; extra: synthetic additions to the entry
# list -- 'col': one more input column that nothing reads, 'term': one more term without an entry (cuts give such terms too)
KERNEL_CASES = {
    'pair': dict(array='pair', Nt=1, Nf=1, Tm=True, Fm=True, dly=True, use_reds=True, compress=False, second=True),
    'pair_f70': dict(array='pair', Nt=3, Nf=70, Tm=False, Fm=False, dly=True, use_reds=False, compress=True, second=True),
    'hex7_red': dict(array=(2, True), Nt=3, Nf=5, Tm=True, Fm=True, dly=True, use_reds=True, compress=True, second=True),
    'hex7_tb': dict(array=(2, True), Nt=3, Nf=5, Tm=False, Fm=True, dly=True, use_reds=True, compress=False, second=True,
                    extra=('col', 'term')),
    'hex7_fb': dict(array=(2, True), Nt=3, Nf=70, Tm=True, Fm=False, dly=True, use_reds=False, compress=True, second=False),
    'hex7_tfb': dict(array=(2, True), Nt=3, Nf=70, Tm=False, Fm=False, dly=True, use_reds=True, compress=True, second=True,
                     setup=dict(max_len=16.0, second_max_len=15.0)),
    'hex7_nodly': dict(array=(2, True), Nt=1, Nf=70, Tm=True, Fm=True, dly=False, use_reds=False, compress=False, second=True),
    'hex7_f1': dict(array=(2, True), Nt=3, Nf=1, Tm=False, Fm=True, dly=True, use_reds=True, compress=True, second=False,
                    extra=('col',)),
    'hex19': dict(array=(3, False), Nt=1, Nf=5, Tm=True, Fm=True, dly=True, use_reds=True, compress=True, second=True,
                  straddle=True),
}


def case_setup(name):
    """(ants, vecs, bls_in, bls_out, case keywords)"""
    c = dict(KERNEL_CASES[name])
    if c['array'] == 'pair':
        ants, vecs = [4, 1], np.array([[0.0, 0.0, 0.0], [14.6, 3.0, 0.0]])
        bls_out = [(1, 4)]
        bls_red = [(1, 4)]
    else:
        ants, vecs = hex_positions(*c['array'])
        bls_out, bls_red = array_bls(ants, vecs)
    return ants, vecs, (bls_red if c['use_reds'] else list(bls_out)), bls_out, c


def straddle(ent, counts, Nterms):
    """pad the lists of three terms with first-order entries (row 0, column 0) so that they hold k SEG - 1, k SEG and
    k SEG + 1 words, and one more to more than WAVES segments (a wave then adds more than one segment sum: a second level
    of the combine); returns the padded entry arrays and the four terms"""
    row, col, conj, a, b = [list(x) for x in ent]
    pick = [int(c) for c in np.argsort(-counts)[:4]]
    for c, want in zip(pick, (-1, 0, 1, None)):
        n = int(counts[c])
        target = (-(-(n + 1) // SEG)) * SEG + want if want is not None else max(n, WAVES * SEG + 1)
        for _ in range(target - n):
            row.append(0); col.append(0); conj.append(0); a.append(c); b.append(-1)
    return tuple(np.array(x, dtype=np.int64) for x in (row, col, conj, a, b)), pick


def case_arrays(c, ent, Nin, Nout, Nterms, seed=0):
    """float32-exact complex128 inputs X, D, data, G of a case"""
    rng = np.random.default_rng([seed, Nin, Nout, Nterms])
    Nt, Nf = c['Nt'], c['Nf']

    def cx(*shape, scale=1.0):
        z = (rng.normal(size=shape) + 1j * rng.normal(size=shape)) * scale
        return z.astype(np.complex64).astype(np.complex128)

    X = cx(Nterms, Nt if c['Tm'] else 1, Nf if c['Fm'] else 1, scale=0.3)
    D = np.exp(1j * rng.uniform(0, 2 * np.pi, size=(Nterms, Nf))).astype(np.complex64).astype(np.complex128) if c['dly'] else None
    return X, D, cx(Nin, Nt, Nf), cx(Nout, Nt, Nf)
