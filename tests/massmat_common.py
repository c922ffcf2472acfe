"""
What the massmat tests share: a float64 numpy restatement of rime_mass_project, rime_mass_drift, the leapfrog and K on the flat
vector, each returning its value AND a running bound on what a computation in the working type T may differ by; the test factors;
the case tables.

The bound is derived, not measured.  With unit roundoff u of T (2^-24, 2^-53) a dot product of m terms, in any order and with or
without fused multiply-adds, differs from the exact one by at most g(m) sum |a_i b_i|, g(m) = m u / (1 - m u) (Higham 2002, 3.1);
an fma or a product by u times its result.  Composed as the kernels compose them, with dX the bound carried by X:
  p' = p - k eps g        dp' = dp + |k eps| dg + u (|p'| + 2 |k eps g|)              (T(k), T(k) * eps and the fma)
  z  = L^T p'             dz_j = sum_i |L_ij| dp'_i + g(n - j) sum_i |L_ij| (|p'_i| + dp'_i);      diagonal: |c| dp' + u |z|
  y  = L z                dy_i = sum_j |L_ij| dz_j + g(i + 1) sum_j |L_ij| (|z_j| + dz_j);          diagonal: |c| dz + u |y|
  q' = q + d eps y        dq' = dq + |d eps| dy + u (|q'| + 2 |d eps y|)
  K  = 1/2 sum z^2        dK = sum (|z| dz + dz^2 / 2) + (E + 32) u K         (the lane's chain of E <= 16 terms in T, then float64)
  a  = sum (q' - f) r     da = sum (dq' |r| + |q' - f| dr + u |q' - f| |r|) + (E + 32) u sum |q' - f| |r|
and the gradient of the quadratic potential U = 1/2 q^T A q, g = A q, by dg = |A| dq + g(n) |A| (|q| + dq).
The restatement itself runs in float64 and rounds like any computation in float64, so what a result in T may differ from IT by is the
bound with u = u_T + 2^-53 (unit()): for float32 the second term is nothing, for float64 it doubles the bound.
"""
import numpy as np

U_ROUND = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
NP_DTYPE = {'f32': np.float32, 'f64': np.float64}
SLACK = 48                                                    # E + 32, E <= 16

# one block: the sizes of the issue, and one that spans several work-groups of both triangular kernels (set by the GPU test from the
# module's strip sizes)
ONE_BLOCK_N = (1, 2, 63, 64, 65, 257)
# mixed layout: (name, kind, n): a diagonal real key of odd length, a dense real key, a dense complex key after an odd offset
MIXED = (('d', 'diag', 37), ('r', 'dense', 45), ('w', 'cdense', 21))


def unit(prec):
    """the unit roundoff the bounds are evaluated with: that of T plus that of the float64 restatement itself"""
    return U_ROUND[prec] + U_ROUND['f64']


def gamma(m, u):
    m = np.asarray(m, dtype=np.float64)
    return m * u / (1.0 - m * u)


def factor(n, seed):
    """L = I + 0.3 tril(randn(n, n)) / sqrt(n): a benign lower-triangular factor"""
    rng = np.random.default_rng(seed)
    return np.eye(n) + 0.3 * np.tril(rng.normal(size=(n, n))) / np.sqrt(n)


def spd(n, seed):
    """a symmetric positive definite matrix with eigenvalues of order one (the quadratic potential)"""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(n, n)) / np.sqrt(n)
    return B @ B.T + 0.5 * np.eye(n)


def covered(blocks, N):
    m = np.zeros(N, dtype=bool)
    for L, off, nrhs in blocks:
        m[off:off + L.shape[0] * nrhs] = True
    return m


def project(blocks, c, p_in, g, eps, kick, u, dp=0.0, dg=0.0):
    """(p_out, dp_out, z, dz) on flat float64 vectors; blocks = [(L float64 (n, n), off, nrhs)]; c, eps arrays or None"""
    N = p_in.size
    c = np.ones(N) if c is None else c
    eps = np.ones(N) if eps is None else eps
    if kick != 0.0:
        t = kick * eps * g
        p = p_in - t
        dp = dp + np.abs(kick * eps) * dg + u * (np.abs(p) + 2 * np.abs(t))
    else:
        p, dp = p_in.copy(), dp + np.zeros(N)
    z = c * p
    dz = np.abs(c) * dp + u * np.abs(z)
    for L, off, nrhs in blocks:
        n = L.shape[0]
        Lt, aLt = np.tril(L).T, np.abs(np.tril(L)).T
        gm = gamma(n - np.arange(n), u)
        for r in range(nrhs):
            s = slice(off + r, off + n * nrhs, nrhs)
            z[s] = Lt @ p[s]
            dz[s] = aLt @ dp[s] + gm * (aLt @ (np.abs(p[s]) + dp[s]))
    return p, dp, z, dz


def drift(blocks, c, z, q_in, eps, drift_, u, dz=0.0, dq=0.0):
    """(q_out, dq_out) on flat float64 vectors"""
    N = z.size
    c = np.ones(N) if c is None else c
    eps = np.ones(N) if eps is None else eps
    dz = dz + np.zeros(N)
    y = c * z
    dy = np.abs(c) * dz + u * np.abs(y)
    for L, off, nrhs in blocks:
        n = L.shape[0]
        Ll, aL = np.tril(L), np.abs(np.tril(L))
        gm = gamma(np.arange(n) + 1, u)
        for r in range(nrhs):
            s = slice(off + r, off + n * nrhs, nrhs)
            y[s] = Ll @ z[s]
            dy[s] = aL @ dz[s] + gm * (aL @ (np.abs(z[s]) + dz[s]))
    t = drift_ * eps * y
    q = q_in + t
    dq = dq + np.abs(drift_ * eps) * dy + u * (np.abs(q) + 2 * np.abs(t))
    return q, dq


def kinetic(z, u, dz=0.0):
    """(K, dK) = 1/2 sum z^2"""
    dz = dz + np.zeros(z.size)
    K = 0.5 * np.sum(z * z)
    return K, np.sum(np.abs(z) * dz + 0.5 * dz * dz) + SLACK * u * K


def projection(q, f, r, u, dq=0.0, dr=0.0):
    """(a, da) = sum (q - f) r"""
    d = q - f
    s = np.sum(np.abs(d) * np.abs(r))
    return np.sum(d * r), np.sum(dq * np.abs(r) + np.abs(d) * dr + dq * dr) + (SLACK + 1) * u * s


def quad_grad(A_of, u):
    """gradient of U = 1/2 sum_k q_k^T A_k q_k on the flat vector: A_of = [(A (n, n), off, nrhs)] covering what moves"""
    def grad(q, dq):
        g, dg = np.zeros(q.size), np.zeros(q.size)
        for A, off, nrhs in A_of:
            n = A.shape[0]
            for r in range(nrhs):
                s = slice(off + r, off + n * nrhs, nrhs)
                g[s] = A @ q[s]
                dg[s] = np.abs(A) @ dq[s] + gamma(n, u) * (np.abs(A) @ (np.abs(q[s]) + dq[s]))
        return g, dg
    return grad


def leapfrog(blocks, c, q, p, grad, eps, Nstep, u, eps_vec=None):
    """Nstep leapfrog steps in the kernels' stage order: returns (q, dq, p, dp, K, dK); eps a float, eps_vec a per-element factor"""
    dq, dp = np.zeros(q.size), np.zeros(p.size)
    stages = [(0.5, 1.0)] + [(1.0, 1.0)] * (Nstep - 1) + [(0.5, 0.0)]
    z = dz = None
    for kick, dr in stages:
        g, dg = grad(q, dq)
        p, dp, z, dz = project(blocks, c, p, g, eps_vec, kick * eps, u, dp, dg)
        if dr:
            q, dq = drift(blocks, c, z, q, eps_vec, dr * eps, u, dz, dq)
    K, dK = kinetic(z, u, dz)
    return q, dq, p, dp, K, dK


def mixed_layout():
    """offsets of MIXED as sampler._Layout places them (a complex key starts on an even element): {name: (off, n, nrhs)}, N"""
    out, n = {}, 0
    for name, kind, m in MIXED:
        nrhs = 2 if kind == 'cdense' else 1
        n += (n & 1) if nrhs == 2 else 0
        out[name] = (n, m, nrhs)
        n += m * nrhs
    return out, n


# ---- the golden file (tests/golden/make_golden_massmat.py -> massmat.npz): keys (name, kind, n), seeds and sizes
GOLDEN_KEYS = (('d', 'diag', 7), ('r', 'dense', 9), ('w', 'cdense', 5))
GOLDEN_SEED, GOLDEN_TENSOR_N, GOLDEN_EPS, GOLDEN_NSTEP, GOLDEN_STEPS, GOLDEN_DEPTH = 2024, 12, 0.45, 5, 6, 4


def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'massmat.npz'))


def golden_layout():
    """{name: (off, n, nrhs)}, N of GOLDEN_KEYS as sampler._Layout places them"""
    out, n = {}, 0
    for name, kind, m in GOLDEN_KEYS:
        nrhs = 2 if kind == 'cdense' else 1
        n += (n & 1) if nrhs == 2 else 0
        out[name] = (n, m, nrhs)
        n += m * nrhs
    return out, n


def golden_pack(G, prefix):
    """the arrays G[prefix + key] as the flat real vector of the layout (a complex key interleaved)"""
    lay, N = golden_layout()
    out = np.zeros(N)
    for k, (off, n, nrhs) in lay.items():
        v = np.asarray(G[prefix + k])
        out[off:off + n * nrhs] = np.stack([v.real, v.imag], axis=-1).ravel() if nrhs == 2 else v.real
    return out


def golden_flat(G):
    """(blocks, c, A_of, q0, p0, N) of the golden ParamDict case for the restatement"""
    lay, N = golden_layout()
    kind = {k: kd for k, kd, _ in GOLDEN_KEYS}
    blocks = [(np.asarray(G['d_L_' + k]), off, nrhs) for k, (off, n, nrhs) in lay.items() if kind[k] != 'diag']
    c = np.ones(N)
    for k, (off, n, nrhs) in lay.items():
        if kind[k] == 'diag':
            c[off:off + n] = G['d_L_' + k]
    A_of = [(np.asarray(G['d_A_' + k]), off, nrhs) for k, (off, n, nrhs) in lay.items()]
    return blocks, c, A_of, golden_pack(G, 'd_q0_'), golden_pack(G, 'd_p0_'), N


def chain_tol(prec):
    """
    Relative tolerance on the Hamiltonians and positions of a golden chain's move: every stage is a composition of dot products of
    at most N terms (the factor, its transpose, the potential's matrix: error N u each relative to the sum of magnitudes), a move
    has at most 2^GOLDEN_DEPTH stages, and the well-conditioned test factors and potentials (eigenvalues of order one) keep the sum
    of magnitudes within a factor of 64 of the result: 64 x stages x N x u.
    """
    _, N = golden_layout()
    return 64 * 2 ** GOLDEN_DEPTH * N * unit(prec)
