"""
Shared by the hmat tests and tests/golden/make_golden_hmat.py: operator trees as plain data (specs of numpy float64 arrays), a
numpy float64 restatement of a spec as a dense matrix, the quantities of the derived error bound, builders that turn a spec
into operators of bayeslim_amd.hmat (or of the reference's hmat, for the generator), the case tables and the recorded
distances of the L-BFGS direction.

A spec is a tuple: ('dense', A) | ('diag', d, size) | ('sparse', shape, U, V or None, Hdiag or None, hermitian) |
('zero', shape) | ('triang', L, lower) | ('T', spec) | ('part', {(i, j): spec}, symmetric) | ('col', [specs]) | ('row', [specs]) |
('hier', A00, A11, A01 or None, A10 or None, sym, scalar or None).

Error bound of a product (derived, not chosen): against the float64 restatement, row i of y = A x computed in a precision of
unit roundoff u by ANY summation order differs by at most (K_i + 2) u (|A| |x|)_i, with |A| the dense matrix of absolute values
(|U| |V| plus |Hdiag| for a low-rank leaf) and K_i the number of columns plus the ranks plus the number of tiles met by row i:
every term passes through at most K_i additions and one product, a low-rank term through both of its chains, and the scale
and scalar products add the 2.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hmat.npz')
_CACHE = {}
U32, U64 = 2.0 ** -24, 2.0 ** -53

# L-BFGS direction with an hmat starting matrix: max|r - r_golden| / max|r_golden| over the four two-loop cases.  The kernel
# path may be at most TLR_FACTOR times as far from the golden as the torch restatement of the reference's recursion in the same
# precision on the CPU: a different but fixed summation order is the only difference.
# Recorded, float32: TLR32_RESTATEMENT (x86-64 CPU; set by 'hier'; diag 1.58e-7, sparse 1.78e-7, part 4.71e-7) and TLR32_KERNEL
# (MI355X; set by 'part'; diag 1.55e-7, sparse 1.25e-7, hier 1.50e-7).  In float64: restatement 7.4e-16, kernel path 4.7e-16.
TLR_FACTOR = 4.0
TLR32_RESTATEMENT = 5.61e-07
TLR32_KERNEL = 1.57e-07
TLR_N, TLR_M = 300, 7
TLR_KINDS = ('diag', 'sparse', 'part', 'hier')


def golden():
    if GOLDEN not in _CACHE:
        with np.load(GOLDEN) as f:
            _CACHE[GOLDEN] = {k: f[k] for k in f.files}
    return _CACHE[GOLDEN]


# ------------------------------------------------------------------------------------------------------------ specs
def _sym(rng, n, scale=1.0):
    a = rng.normal(size=(n, n)) * scale
    return (a + a.T) / 2


def tree_specs():
    """name -> spec, the same arrays on every call"""
    rng = np.random.default_rng(2024)
    n = lambda *s: rng.normal(size=s)
    part3 = ('part', {(1, 1): ('dense', _sym(rng, 257)), (2, 2): ('dense', _sym(rng, 130)),
                      (3, 3): ('sparse', (600, 600), n(600, 33) / 6, None, rng.uniform(0.5, 2, 600), True),
                      (1, 2): ('dense', n(257, 130)), (1, 3): ('sparse', (257, 600), n(257, 1), n(1, 600), None, False)}, True)
    inner = ('hier', ('dense', _sym(rng, 65)), ('diag', rng.uniform(0.5, 2, 63), 63),
             ('sparse', (65, 63), n(65, 3), n(3, 63), None, False), None, True, None)
    hier2 = ('hier', inner, ('dense', _sym(rng, 200)), ('sparse', (128, 200), n(128, 5), n(5, 200), None, False), None, True, 0.5)
    row = ('row', [('dense', n(70, 30)), ('diag', rng.uniform(0.5, 2, 70), 70), ('sparse', (70, 40), n(70, 2), n(2, 40), None, False)])
    col = ('col', [('dense', n(30, 70)), ('diag', np.array([1.7]), 70), ('zero', (20, 70)), ('triang', np.tril(n(70, 70)), True),
                   ('T', ('dense', n(70, 1)))])
    rect = ('sparse', (90, 50), n(90, 4), n(4, 50), rng.uniform(0.5, 2, 50), False)
    tiny = ('part', {(1, 1): ('dense', n(1, 1)), (2, 2): ('diag', np.array([0.3]), 5), (1, 2): ('zero', (1, 5))}, False)
    return dict(part3=part3, hier2=hier2, row=row, col=col, rect=rect, tiny=tiny)


def shape(spec):
    k = spec[0]
    if k in ('dense', 'triang'):
        return spec[1].shape
    if k == 'diag':
        return (spec[2], spec[2])
    if k in ('sparse', 'zero'):
        return tuple(spec[1])
    if k == 'T':
        return shape(spec[1])[::-1]
    return _layout(spec, lambda s: np.zeros(shape(s))).shape


def _layout(spec, leaf):
    """assemble a container from leaf(child) matrices"""
    k = spec[0]
    if k == 'col':
        return np.concatenate([leaf(s) for s in spec[1]], axis=0)
    if k == 'row':
        return np.concatenate([leaf(s) for s in spec[1]], axis=1)
    if k == 'part':
        blocks, symmetric = spec[1], spec[2]
        keys = sorted(b for b in blocks if b[0] == b[1])
        rows = []
        for i in keys:
            r = []
            for j in keys:
                bk = (i[0], j[1])
                if bk in blocks:
                    r.append(leaf(blocks[bk]))
                elif symmetric and bk[::-1] in blocks:
                    r.append(leaf(('T', blocks[bk[::-1]])))
                else:
                    r.append(leaf(('zero', (shape(blocks[i])[0], shape(blocks[j])[1]))))
            rows.append(np.concatenate(r, axis=1))
        return np.concatenate(rows, axis=0)
    if k == 'hier':
        A00, A11, A01, A10, sym, scalar = spec[1:]
        if sym:
            A01 = ('T', A10) if A01 is None and A10 is not None else A01
            A10 = ('T', A01) if A10 is None and A01 is not None else A10
        z = lambda a, b: ('zero', (shape(a)[0], shape(b)[1]))
        out = np.block([[leaf(A00), leaf(A01 if A01 is not None else z(A00, A11))],
                        [leaf(A10 if A10 is not None else z(A11, A00)), leaf(A11)]])
        return out
    raise ValueError(k)


def dense(spec, absolute=False):
    """the operator of a spec as a float64 matrix; absolute: the matrix |A| of the bound"""
    f = np.abs if absolute else (lambda a: a)
    k = spec[0]
    if k == 'dense':
        return f(spec[1])
    if k == 'triang':
        return f(np.tril(spec[1]) if spec[2] else np.triu(spec[1]))
    if k == 'diag':
        return np.diag(f(np.broadcast_to(spec[1], (spec[2],))))
    if k == 'zero':
        return np.zeros(spec[1])
    if k == 'T':
        return dense(spec[1], absolute).T
    if k == 'sparse':
        _, shp, U, V, Hdiag, herm = spec
        out = f(U) @ f(U.T if herm else V)
        if Hdiag is not None:
            idx = np.arange(len(Hdiag))
            out[idx, idx] += f(Hdiag)
        return out
    out = _layout(spec, lambda s: dense(s, absolute))
    if k == 'hier' and spec[6] is not None:
        out = out * (abs(spec[6]) if absolute else spec[6])
    return out


def row_terms(spec):
    """K of the bound as a matrix of the operator's shape summed over columns later: per row, columns + ranks + tiles"""
    k = spec[0]
    R, C = shape(spec)
    if k in ('dense', 'triang'):
        return np.full(R, C + 1.0)
    if k == 'diag':
        return np.full(R, 2.0)
    if k == 'zero':
        return np.zeros(R)
    if k == 'sparse':
        out = np.full(R, C + spec[2].shape[1] + 2.0)
        if spec[4] is not None:
            out[:len(spec[4])] += 2.0
        return out
    if k == 'T':
        inner = spec[1]
        if inner[0] == 'T':
            return row_terms(inner[1])
        if inner[0] in ('dense', 'triang', 'diag', 'zero', 'sparse'):
            ri, ci = shape(inner)
            flipped = {'dense': ('dense', np.zeros((ci, ri))), 'triang': ('dense', np.zeros((ci, ri))), 'diag': inner,
                       'zero': ('zero', (ci, ri))}.get(inner[0])
            if inner[0] == 'sparse':
                flipped = ('sparse', (ci, ri), np.zeros((ci, inner[2].shape[1])), None, inner[4], False)
            return row_terms(flipped)
        raise ValueError('transposed containers are bounded through transpose_spec')
    return _layout(spec, lambda s: np.tile(row_terms(s)[:, None], (1, max(shape(s)[1], 1)))[:, :shape(s)[1]]
                   / max(shape(s)[1], 1)).sum(axis=1)


def transpose_spec(spec):
    """the spec of the transposed operator with the transposition pushed down to the leaves"""
    k = spec[0]
    if k == 'T':
        return spec[1]
    if k == 'col':
        return ('row', [transpose_spec(s) for s in spec[1]])
    if k == 'row':
        return ('col', [transpose_spec(s) for s in spec[1]])
    if k == 'part':
        full = {}
        keys = sorted(b for b in spec[1] if b[0] == b[1])
        for i in keys:
            for j in keys:
                bk = (i[0], j[1])
                if bk in spec[1]:
                    full[bk[::-1]] = transpose_spec(spec[1][bk])
                elif spec[2] and bk[::-1] in spec[1]:
                    full[bk[::-1]] = spec[1][bk[::-1]]
        return ('part', full, False)
    if k == 'hier':
        A00, A11, A01, A10, sym, scalar = spec[1:]
        t = lambda a: None if a is None else transpose_spec(a)
        if sym:
            A01 = ('T', A10) if A01 is None and A10 is not None else A01
            A10 = ('T', A01) if A10 is None and A01 is not None else A10
        return ('hier', t(A00), t(A11), t(A10), t(A01), False, scalar)
    return ('T', spec)


def bound(spec, x, u, transpose=False):
    """(K + 2) u |A| |x| for x [N] or [N, M], real or complex (|x| then bounds both components)"""
    sp = transpose_spec(spec) if transpose else spec
    absx = np.maximum(np.abs(x.real), np.abs(x.imag)) if np.iscomplexobj(x) else np.abs(x)
    K = row_terms(sp)
    ax = dense(sp, absolute=True) @ absx
    return (K + 2.0).reshape((-1,) + (1,) * (ax.ndim - 1)) * u * ax


def within(y, ref, bnd):
    """every component of y - ref within the bound; returns the largest ratio for printing"""
    d = y - ref
    parts = [np.abs(d.real), np.abs(d.imag)] if np.iscomplexobj(d) else [np.abs(d)]
    worst = 0.0
    for p in parts:
        ok = p <= bnd
        if not ok.all():
            return False, float((p[~ok] / np.maximum(bnd[~ok], 1e-300)).max())
        nz = bnd > 0
        worst = max(worst, float((p[nz] / bnd[nz]).max()) if nz.any() else 0.0)
    return True, worst


# ------------------------------------------------------------------------------------------------------------ builders
def build(spec, mod, tensor):
    """the operator of a spec from the classes of module `mod`; tensor(array) makes the tensors"""
    k = spec[0]
    b = lambda s: None if s is None else build(s, mod, tensor)
    if k == 'dense':
        return mod.DenseMat(tensor(spec[1]))
    if k == 'diag':
        return mod.DiagMat(tensor(spec[1]), spec[2])
    if k == 'zero':
        t0 = tensor(np.zeros(1))
        return mod.ZeroMat(tuple(spec[1]), dtype=t0.dtype, device=t0.device)
    if k == 'triang':
        return mod.TriangMat(tensor(spec[1]), lower=spec[2])
    if k == 'T':
        return mod.TransposedMat(b(spec[1]))
    if k == 'sparse':
        _, shp, U, V, Hdiag, herm = spec
        return mod.SparseMat(tuple(shp), tensor(U), V=None if V is None else tensor(V), Hdiag=None if Hdiag is None else tensor(Hdiag),
                             hermitian=herm)
    if k == 'col':
        return mod.MatColumn([b(s) for s in spec[1]])
    if k == 'row':
        return mod.MatRow([b(s) for s in spec[1]])
    if k == 'part':
        return mod.PartitionedMat({key: b(s) for key, s in spec[1].items()}, symmetric=spec[2])
    if k == 'hier':
        A00, A11, A01, A10, sym, scalar = spec[1:]
        return mod.HierMat(b(A00), b(A11), A01=b(A01), A10=b(A10), sym=sym, scalar=scalar)
    raise ValueError(k)


def rhs(N, kind, seed=7):
    rng = np.random.default_rng(seed + N)
    if kind == 'real':
        return rng.normal(size=N)
    if kind == 'complex':
        return rng.normal(size=N) + 1j * rng.normal(size=N)
    if kind == 'mat3':
        return rng.normal(size=(N, 3))
    raise ValueError(kind)


RHS_KINDS = ('real', 'complex', 'mat3')


# ------------------------------------------------------------------------------------------------------------ two-loop cases
def tlr_problem():
    """(s, y [m, N], vec [N], rho [m], {kind: spec}) of the L-BFGS direction cases: a positive definite quadratic's pairs"""
    rng = np.random.default_rng(99)
    N, m = TLR_N, TLR_M
    w = rng.normal(size=(N, 3)) / np.sqrt(N)
    u = rng.uniform(0.5, 2.0, N)
    s = rng.normal(size=(m, N))
    y = s * u + (s @ w) @ w.T
    vec = rng.normal(size=N)
    rho = 1.0 / np.einsum('ij,ij->i', s, y)
    n0 = 120
    a = rng.normal(size=(n0, n0)) / np.sqrt(n0)
    d0 = a @ a.T + np.eye(n0)
    sp = ('sparse', (N - n0, N - n0), rng.normal(size=(N - n0, 4)) / 10, None, 1 / u[n0:], True)
    off = ('sparse', (n0, N - n0), rng.normal(size=(n0, 2)) / 10, rng.normal(size=(2, N - n0)) / 10, None, False)
    specs = dict(diag=('diag', 1 / u, N),
                 sparse=('sparse', (N, N), rng.normal(size=(N, 5)) / 10, None, 1 / u, True),
                 part=('part', {(1, 1): ('dense', d0), (2, 2): sp, (1, 2): off}, True),
                 hier=('hier', ('dense', d0), sp, off, None, True, 0.8))
    return s, y, vec, rho, specs


def two_loop_torch(vec, s, y, rho, H0):
    """the reference's two-loop recursion restated in torch, in its operation order, in the dtype of its arguments; H0 a callable"""
    q = vec.clone()
    m = len(s)
    alpha = [None] * m
    for i in reversed(range(m)):
        alpha[i] = rho[i] * (s[i] @ q)
        q = q - alpha[i] * y[i]
    r = H0(q)
    for i in range(m):
        beta = rho[i] * (y[i] @ r)
        r = r + s[i] * (alpha[i] - beta)
    return r
