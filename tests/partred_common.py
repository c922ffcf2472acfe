"""
Shared by tests/test_partred_host.py, tests/test_partred_gpu.py and tests/golden/make_golden_partred.py: a float64 numpy
restatement of the sparse mixing of calibration.PartialRedVisInflate (the forward and both gradients), written from the
formulas and not from the kernel, the case tables, and the derived accuracy bound.

Formulas.  Entry e = (row i_e, column j_e) with the real coefficient c_e; V (Npol, Npol, Nin, Nt, Nf), G (Npol, Npol, Nout, Nt, Nf):
    out[:, :, i]  = sum over the entries of row i of     c_e V[:, :, j_e]
    gV[:, :, j]   = sum over the entries of column j of  c_e G[:, :, i_e]
    gc[e]         = sum over (p, q, t, f) of  Re V[p, q, j_e, t, f] Re G[p, q, i_e, t, f] + Im V Im G
Cotangents follow torch's convention for complex tensors.

The bound (derived, not measured; fixed by the design of the kernel, not by its results).  u = 2^-24 or 2^-53,
gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  c is real, so the real and
the imaginary component of out and gV are separate real sums, and per real component
    |error| <= gamma_n(u) M
with M the same sum over the absolute values of the components (evaluate() on |c|, |Re V| + i |Im V|, |Re G| + i |Im G|) and n
the roundings on the longest chain to an element (csrc/partred.hip):
    forward  one FMA per term onto the accumulator, in list order:  n = L_row, the longest row list
    gV       a wave adds ceil(L_col / WAVES) members by one FMA each, wave 0 the WAVES - 1 other partial sums:
             n = ceil(L_col / WAVES) + WAVES - 1
    gc       a thread adds ceil(L / THREADS) elements, two FMAs each, in T: 2 ceil(L / THREADS); then in float64 the butterfly
             log2(64) = 6 and the waves THREADS / 64 - 1 = 3: 9 at 2^-53; one rounding to T at the end:
             (1 + gamma_{2 ceil(L / THREADS) + 1}(u)) (1 + gamma_9(2^-53)) - 1,   L = Npol^2 Nt Nf
The restatement multiplies and adds in float64 without FMA, entry by entry: 2 L_row, 2 L_col, and for gc a product per term
and numpy's sum of 2 L terms in an order of its own, at most 2 L + 1 on a chain.  A comparison counts both sides:
gamma_n(u_kernel) + gamma_n'(2^-53).  Against the reference-generated fixture (float64; dense matrix and einsum over all Nin
columns, any order) the other side's counts are Nin + 2 (out), Nout + 2 (gV: the transposed product) and 2 L + 2 (gc: the
gradient of the dense matrix, a complex product per element).  Where the cotangent is computed from the output (the fixture's
loss sum w |out|^2, G = 2 w out) its absolute values come from the forward's M, |G| <= 2 w M_out, and the forward's roundings of
both sides + 2 are added to the count of the gradient.  Where the gradient passes on through the response R (chain rule:
gparams = gc R'(params + p0)) M is multiplied by |R'| and CHAIN = 4 roundings per side are added (R' to within two
roundings, the product one, one spare).  The tests assert error / bound <= 1 for every component and print the worst ratio.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
WAVES, COLS, THREADS, ECH, UNROLL = 4, 64, 256, 4, 4      # csrc/partred.hip: PR_WAVES, PR_COLS, PR_THREADS, PR_ECH, #pragma unroll
NT, NF = 3, 5                                             # the fixture
CHAIN = 4
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(HERE, 'golden', 'partred.npz')) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


# fixture cases: `lists` is bl2red[bl] for the baselines of new_bls in their order (an int: a list of one); Nin is the length
# of the input's baseline axis = largest column + 1; R names a torch function; p0 / params: random (True) or absent / default
NEW_BLS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
GOLDEN_CASES = {
    'p1_sorted': dict(Npol=1, new_bls=NEW_BLS, lists=[[0], [0, 1], [1, 2, 4], [3], [2, 3], [0, 2, 4]], params=False, p0=False, R=None),
    'p2_unsorted': dict(Npol=2, new_bls=NEW_BLS[:5], lists=[[3, 0, 2], 1, [5, 4], 4, [2, 0]], params=True, p0=False, R=None),
    'p1_exp': dict(Npol=1, new_bls=NEW_BLS, lists=[[1, 0], [5], [0, 2, 1], 2, [5, 4, 0], [1]], params=True, p0=True, R='exp'),
}
ANTS = [0, 1, 2, 3]
ANTVECS = np.array([[0.0, 0.0, 0.0], [14.6, 0.0, 0.0], [7.3, 12.6, 0.0], [21.9, 12.6, 0.1]])
RESPONSES = {None: (lambda x: x, lambda x: np.ones_like(x)), 'exp': (np.exp, np.exp)}     # name -> (R, R') in numpy


def entry_list(lists):
    """(rows, cols, Nred) of the entries in the module's order: baseline by baseline, each list as given"""
    rows, cols, Nred = [], [], []
    for i, red in enumerate(lists):
        red = [int(red)] if isinstance(red, (int, np.integer)) else [int(r) for r in red]
        rows += [i] * len(red)
        cols += red
        Nred += [len(red)] * len(red)
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(Nred, dtype=np.int64)


def build_plan(rows, cols, Nout, Nin):
    """the tables of ops.PartRedPlan with explicit loops"""
    byrow, bycol = [[] for _ in range(Nout)], [[] for _ in range(Nin)]
    for e in range(len(rows)):
        byrow[rows[e]].append(e)
        bycol[cols[e]].append(e)
    csr = lambda lists: np.cumsum([0] + [len(x) for x in lists]).astype(np.int32)
    flat = lambda lists: np.array([x for lst in lists for x in lst], dtype=np.int32)
    assert (flat(byrow) == np.arange(len(rows))).all()
    return dict(roff=csr(byrow), col=np.asarray(cols, dtype=np.int32), row=np.asarray(rows, dtype=np.int32), coff=csr(bycol),
                cmem=flat(bycol), Lrow=max(map(len, byrow)), Lcol=max(map(len, bycol)))


def evaluate(c, V, rows, cols, Nout, G=None):
    """c (Nnz,) real, V (NP, NP, Nin, Nt, Nf), G (NP, NP, Nout, Nt, Nf) or None -> (out, gV, gc); called with the absolute
    values of the components of every input it returns the M of the bound"""
    V = np.asarray(V, dtype=np.complex128)
    c = np.asarray(c, dtype=np.float64)
    out = np.zeros(V.shape[:2] + (Nout,) + V.shape[3:], dtype=np.complex128)
    for e in range(len(rows)):
        out[:, :, rows[e]] += c[e] * V[:, :, cols[e]]
    if G is None:
        return out, None, None
    G = np.asarray(G, dtype=np.complex128)
    gV = np.zeros(V.shape, dtype=np.complex128)
    gc = np.zeros(len(rows), dtype=np.float64)
    for e in range(len(rows)):
        gV[:, :, cols[e]] += c[e] * G[:, :, rows[e]]
        v, g = V[:, :, cols[e]], G[:, :, rows[e]]
        gc[e] = np.sum(np.stack([v.real * g.real, v.imag * g.imag]))
    return out, gV, gc


def cabs(x):
    """|Re x| + i |Im x|"""
    return None if x is None else np.abs(x.real) + 1j * np.abs(x.imag)


def magnitudes(c, V, rows, cols, Nout, G=None):
    """(M_out, M_gV) complex arrays whose components are the M of the components, M_gc real"""
    return evaluate(np.abs(c), cabs(np.asarray(V, dtype=np.complex128)), rows, cols, Nout, cabs(G))


def gamma(n, u):
    return n * u / (1 - n * u)


def roundings(P, L, Nout, Nin):
    """roundings of (forward, gV, gc) per side as counted in the module docstring: dict side -> (n_out, n_gV, n_gc); the gc
    entry of the kernel is the pair (count in T, count in float64)"""
    return dict(kernel=(P['Lrow'], -(-P['Lcol'] // WAVES) + WAVES - 1, (2 * -(-L // THREADS) + 1, 9)),
                numpy=(2 * P['Lrow'], 2 * P['Lcol'], 2 * L + 1),
                fixture=(Nin + 2, Nout + 2, 2 * L + 2))


def rel_kernel(n, prec, extra=0):
    """relative bound of the kernel's side: gamma_n(u), or for the (T, float64) pair of gc the product form; extra: further
    roundings in T"""
    if isinstance(n, tuple):
        return (1 + gamma(n[0] + extra, U[prec])) * (1 + gamma(n[1], U['f64'])) - 1
    return gamma(n + extra, U[prec])


def bound(M, n_kernel, prec, n_other, extra=0):
    """(kernel side in `prec` + other side in float64) * M; extra: roundings added to both sides"""
    M = np.asarray(M)
    rel = rel_kernel(n_kernel, prec, extra) + gamma(n_other + extra, U['f64'])
    return rel * M.real + 1j * rel * M.imag if np.iscomplexobj(M) else rel * M


def ratio(got, want, bnd):
    """worst |got - want| / bound over the real components; a zero bound demands equality (ratio 0 or inf)"""
    got, want, bnd = np.asarray(got), np.asarray(want), np.asarray(bnd)
    worst = 0.0
    for part in (('real', 'imag') if np.iscomplexobj(want) else ('real',)):
        e = np.abs(getattr(got, part).astype(np.float64) - getattr(want, part))
        b = getattr(bnd, part)
        r = np.where(b > 0, e / np.where(b > 0, b, 1), np.where(e == 0, 0.0, np.inf))
        worst = max(worst, float(r.max()))
    return worst


# kernel cases: lists as in GOLDEN_CASES (callables build the long ones), Nin, Npol, Nt, Nf
def _long_row():
    return [list(range(ECH + 1)), [0], [ECH, 2]]                      # a row one longer than the entry chunk of gc


def _long_col():
    n = WAVES * UNROLL + 3                                            # 19 members in column 1: more than waves x unroll
    return [[1]] * 2 + [[0, 1]] + [[1, 2]] * (n - 3)


KERNEL_CASES = {
    'one': dict(Npol=1, Nt=1, Nf=1, Nin=3, lists=[[0, 2], [1], [2, 1, 0]]),                    # Nt Nf = 1
    'f67': dict(Npol=1, Nt=2, Nf=67, Nin=4, lists=[[0, 1], [3, 2, 1], 2, [1, 3]]),             # crosses a 64-column tile
    'p2_f100': dict(Npol=2, Nt=3, Nf=100, Nin=3, lists=[[2, 0], [1], [0, 1, 2]]),              # L = 1200: several sweeps of a block
    'empty_row': dict(Npol=1, Nt=3, Nf=5, Nin=3, lists=[[0, 1], [], [2], []]),                 # rows 1 and 3: exactly 0
    'long_row': dict(Npol=1, Nt=3, Nf=5, Nin=ECH + 1, lists=_long_row),
    'empty_col': dict(Npol=2, Nt=3, Nf=5, Nin=5, lists=[[0, 4], [2], [4, 0]]),                 # columns 1 and 3: gradient exactly 0
    'long_col': dict(Npol=1, Nt=2, Nf=40, Nin=3, lists=_long_col),
}


def case_lists(c):
    return c['lists']() if callable(c['lists']) else c['lists']


def case_arrays(name, Npol, Nin, Nout, Nnz, Nt, Nf, seed=0):
    """float32-exact inputs c (float64), V, G (complex128) of a case"""
    rng = np.random.default_rng([seed, Nin, Nout, Nnz, Nt, Nf])

    def cx(*shape):
        z = rng.normal(size=shape) + 1j * rng.normal(size=shape)
        return z.astype(np.complex64).astype(np.complex128)

    c = rng.uniform(-1.0, 1.0, size=Nnz).astype(np.float32).astype(np.float64)
    return c, cx(Npol, Npol, Nin, Nt, Nf), cx(Npol, Npol, Nout, Nt, Nf)
