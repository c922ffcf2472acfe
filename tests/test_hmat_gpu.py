"""
GPU checks of the operator layer (csrc/hmat.hip through bayeslim_amd/hmat.py): single tiles in both forms over the shapes,
leading dimensions, misaligned bases, right-hand-side counts and dtypes of the case table, the operator trees of hmat_common
against the float64 restatement and the golden at the derived bound, bit identity, the solves by residual, and the L-BFGS
direction with an hmat starting matrix.
"""
import numpy as np
import pytest
import torch

import hmat_common as hc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = (1, 3, 63, 64, 65, 257, 1030)
DT = {'f32': (torch.float32, hc.U32), 'f64': (torch.float64, hc.U64)}


def dev(dtype):
    return lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


def to_np(t):
    return t.detach().cpu().numpy().astype(np.complex128 if t.is_complex() else np.float64)


@pytest.fixture(scope='module')
def pool():
    rng = np.random.default_rng(11)
    return rng.normal(size=(1030, 1033)), rng.normal(size=(1030, 5))


@pytest.mark.parametrize('nrhs', [1, 2, 3, 5])
@pytest.mark.parametrize('form', ['N', 'T'])
@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_single_tiles(pool, prec, form, nrhs):
    """every (rows, cols) of SIZES^2 with ld = cols and cols + 3 and a base offset of 0 and 1 element: the bound, and the same
    bits for all four layouts"""
    from bayeslim_amd import hmat
    dtype, u = DT[prec]
    Apool, Xpool = pool
    for rows in SIZES:
        for cols in SIZES:
            A = Apool[:rows, :cols].astype(np.float32 if prec == 'f32' else np.float64).astype(np.float64)
            nin = rows if form == 'T' else cols
            x = Xpool[:nin, :nrhs].astype(np.float32 if prec == 'f32' else np.float64).astype(np.float64)
            M = A.T if form == 'T' else A
            xv = x[:, 0] if nrhs == 1 else x
            ref, bnd = M @ xv, (nin + 1 + 2) * u * (np.abs(M) @ np.abs(xv))
            xd = dev(dtype)(xv)
            outs = []
            for ld in (cols, cols + 3):
                for off in (0, 1):
                    buf = torch.zeros(rows * ld + 1 + 4, dtype=dtype, device=DEV)
                    view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
                    view.copy_(dev(dtype)(A))
                    assert view.data_ptr() == buf.data_ptr() + off * buf.element_size()
                    op = hmat.DenseMat(view)
                    y = op.mat_vec_mul(xd, transpose=(form == 'T')) if nrhs == 1 else op.mat_mat_mul(xd, transpose=(form == 'T'))
                    p = hmat._plan(op, dtype, torch.device(DEV), form == 'T')
                    assert p.tiles[0]['ld'] == ld and p.tiles[0]['a'] == view.data_ptr()     # the view itself, no copy
                    outs.append(y)
                    ok, worst = hc.within(to_np(y), ref, bnd)
                    assert ok, (rows, cols, ld, off, worst)
            assert all(torch.equal(outs[0], o) for o in outs[1:]), (rows, cols)


def _cases():
    return [(name, tr, kind) for name in hc.tree_specs() for tr in (False, True) for kind in hc.RHS_KINDS]


@pytest.fixture(scope='module')
def specs():
    return hc.tree_specs()


@pytest.mark.parametrize('name,tr,kind', _cases())
@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_trees(specs, prec, name, tr, kind):
    from bayeslim_amd import hmat
    dtype, u = DT[prec]
    spec = specs[name]
    # the operator of the arrays as rounded to the dtype, so that the bound covers the arithmetic alone
    rnd = lambda a: a.astype(np.float32).astype(np.float64) if prec == 'f32' else a
    spec_r = _map_arrays(spec, rnd)
    A = hc.dense(spec_r)
    M = A.T if tr else A
    x = hc.rhs(M.shape[1], kind)
    x = (rnd(x.real) + 1j * rnd(x.imag)) if np.iscomplexobj(x) else rnd(x)
    op = hc.build(spec_r, hmat, dev(dtype))
    cdt = {torch.float32: torch.complex64, torch.float64: torch.complex128}[dtype]
    xd = torch.as_tensor(x).to(DEV, cdt if np.iscomplexobj(x) else dtype)
    y = op.mat_vec_mul(xd, transpose=tr) if xd.ndim == 1 else op.mat_mat_mul(xd, transpose=tr)
    bnd = hc.bound(spec_r, x, u, transpose=tr)
    ok, worst = hc.within(to_np(y), M @ x, bnd)
    print('%s %s %s %s: worst ratio to the bound %.3f' % (name, 'T' if tr else 'N', kind, prec, worst))
    assert ok, worst
    assert torch.equal(y, op(xd, transpose=tr))                                    # the same call twice: the same bits
    key = '%s_%s_%s' % (name, 'T' if tr else 'N', kind)
    if prec == 'f64' and key in hc.golden():
        ok, worst = hc.within(to_np(y), hc.golden()[key], bnd)
        assert ok, worst
    # out= accumulates
    out = torch.ones_like(y)
    res = op(xd, transpose=tr, out=out)
    assert res is out
    ok, worst = hc.within(to_np(out) - 1.0, M @ x, bnd + u * (np.abs(M @ x) + 1))
    assert ok, worst
    # to_dense and the operator applied to the identity both give the restatement's matrix, at the bound of that product
    if kind == 'real' and M.shape[1] <= 400:
        eye = np.eye(M.shape[1])
        bnd_eye = hc.bound(spec_r, eye, u, transpose=tr)
        applied = op.mat_mat_mul(torch.eye(M.shape[1], dtype=dtype, device=DEV), transpose=tr)
        assert hc.within(to_np(applied), M, bnd_eye)[0]
        assert hc.within(to_np(op.to_dense(transpose=tr)), M, bnd_eye)[0]


def _map_arrays(spec, f):
    if isinstance(spec, tuple):
        return tuple(_map_arrays(s, f) for s in spec)
    if isinstance(spec, list):
        return [_map_arrays(s, f) for s in spec]
    if isinstance(spec, dict):
        return {k: _map_arrays(s, f) for k, s in spec.items()}
    if isinstance(spec, np.ndarray):
        return f(spec)
    return spec


def test_tables_mix_tiles_in_one_range_and_straddle_ranges(specs):
    from bayeslim_amd import hmat
    p = hmat._plan(hc.build(specs['hier2'], hmat, dev(torch.float64)), torch.float64, torch.device(DEV), False)
    r0 = p.ranges[0]
    kinds0 = [p.tiles[i]['flags'] for i in p.ids[r0[3]:r0[3] + r0[4]]]
    assert any(f & hmat.DIAG for f in kinds0) and any(f == 0 for f in kinds0)
    r1 = [r for r in p.ranges[p.stage_first[1]:] if r[1] == 0][0]                     # the low-rank tiles of the same rows
    assert r1[4] >= 2 and all(p.tiles[i]['flags'] & hmat.SRC_SCRATCH for i in p.ids[r1[3]:r1[3] + r1[4]])
    p = hmat._plan(hc.build(specs['part3'], hmat, dev(torch.float64)), torch.float64, torch.device(DEV), False)
    assert 0 in p.ids[p.ranges[0][3]:][:p.ranges[0][4]] and 0 in p.ids[p.ranges[1][3]:][:p.ranges[1][4]]   # 257 rows: two ranges
    ranks = {t['cols'] if t['flags'] & hmat.TRANS else t['rows'] for t in p.tiles if t['dst_scratch']}
    assert p.nstages == 2 and sorted(ranks) == [1, 33]


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_rows_do_not_depend_on_other_tiles_and_scalar(prec):
    from bayeslim_amd import hmat
    dtype, u = DT[prec]
    rng = np.random.default_rng(8)
    T = dev(dtype)
    D1, D2, D3, B = T(rng.normal(size=(100, 100))), T(rng.normal(size=(90, 90))), T(rng.normal(size=(90, 90))), T(rng.normal(size=(90, 100)))
    x = T(rng.normal(size=190))
    a = hmat.PartitionedMat({(1, 1): hmat.DenseMat(D1), (2, 2): hmat.DenseMat(D2)}, symmetric=False)
    b = hmat.PartitionedMat({(1, 1): hmat.DenseMat(D1), (2, 2): hmat.SparseMat((90, 90), D3[:, :3].contiguous(), hermitian=True,
                                                                                 Hdiag=D3[0].contiguous()),
                             (2, 1): hmat.DenseMat(B)}, symmetric=False)
    ya, yb = a(x), b(x)
    assert torch.equal(ya[:100], yb[:100]) and not torch.equal(ya[100:], yb[100:])
    assert torch.equal(ya[:100], hmat.DenseMat(D1)(x[:100]))
    ys = hmat._apply(a, x, scalar=0.25)
    assert torch.equal(ys, ya * 0.25)                                               # a power of two: exact
    one = hmat.DenseMat(T(np.array([[3.0]])))
    assert float(one(T(np.array([2.0])))[0]) == 6.0
    z = hmat.ZeroMat((4, 7))
    assert torch.equal(z(T(np.ones(7))), torch.zeros(4, dtype=dtype, device=DEV))
    assert torch.equal(hmat.DiagMat(T(np.array([0.5])), 6)(T(np.arange(6.0))), T(np.arange(6.0) / 2))


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('hermitian', [True, False])
def test_long_low_rank_leaf_is_split_into_partial_sums(prec, hermitian):
    """an input longer than hmat.SPLIT: partial products per piece, added by unit diagonal tiles, then the left factor (three
    stages); the bound with K = columns + rank + tiles (pieces + unit tiles + left factor + Hdiag), both directions"""
    from bayeslim_amd import hmat
    dtype, u = DT[prec]
    rng = np.random.default_rng(31)
    rnd = lambda a: a.astype(np.float32).astype(np.float64) if prec == 'f32' else a
    N, R, k = 9001, 9001 if hermitian else 300, 5
    U, V, d = rnd(rng.normal(size=(R, k))), rnd(rng.normal(size=(k, N))), rnd(rng.uniform(0.5, 2, min(N, R)))
    x = rnd(rng.normal(size=(N, 2)))
    T = dev(dtype)
    op = hmat.SparseMat((R, N), T(U), V=None if hermitian else T(V), Hdiag=T(d), hermitian=hermitian)
    Vm = U.T if hermitian else V
    A = U @ Vm
    A[np.arange(len(d)), np.arange(len(d))] += d
    absA = np.abs(U) @ np.abs(Vm)
    absA[np.arange(len(d)), np.arange(len(d))] += np.abs(d)
    p = hmat._plan(op, dtype, torch.device(DEV), False)
    pieces = -(-N // hmat.SPLIT)
    assert pieces == 3 and p.nstages == 3 and len(p.tiles) == 2 * pieces + 2 and p.scratch_rows == k * (pieces + 1)
    for tr in (False, True):
        M, aM = (A.T, absA.T) if tr else (A, absA)
        xx = x[:M.shape[1]]
        pcs = -(-M.shape[1] // hmat.SPLIT)
        y = op.mat_mat_mul(T(xx), transpose=tr)
        bnd = (M.shape[1] + k + 2 * pcs + 2 + 2) * u * (aM @ np.abs(xx))
        ok, worst = hc.within(to_np(y), M @ xx, bnd)
        assert ok, (tr, worst)
        assert torch.equal(y, op.mat_mat_mul(T(xx), transpose=tr))


def test_leafwise_trees_and_elementwise_leaves():
    from bayeslim_amd import hmat
    T = dev(torch.float64)
    rng = np.random.default_rng(4)
    A, v = rng.normal(size=(6, 6)), rng.normal(size=6)
    col = hmat.MatColumn([hmat.DenseMat(T(A)), hmat.OneMat((3, 6), 2.0, dtype=torch.float64, device=DEV)])
    want = np.concatenate([A @ v, np.full(3, 2.0 * v.sum())])
    assert np.allclose(to_np(col(T(v))), want, rtol=1e-13)
    assert np.allclose(to_np(col(T(np.ones(9)), transpose=True)), A.T @ np.ones(6) + 2.0 * 3, rtol=1e-13)
    h = hmat.HadamardMat(T(A))
    assert np.allclose(to_np(h(T(A))), A * A)


@pytest.mark.parametrize('tag', ['real', 'complex'])
def test_solves_by_residual(tag):
    from bayeslim_amd import hmat
    rng = np.random.default_rng(5)
    n, n0 = 100, 40
    a = rng.normal(size=(n, n)) / np.sqrt(n)
    L = np.linalg.cholesky(a @ a.T + np.eye(n))
    b = rng.normal(size=n)
    bc = rng.normal(size=n) + 1j * rng.normal(size=n)
    v = b if tag == 'real' else bc
    T = dev(torch.float64)
    vd = torch.as_tensor(v).to(DEV)
    u = hc.U64

    def residual_ok(Lm, z, rhs_):
        # a complex right-hand side is two real solves: each component by its own residual
        if np.iscomplexobj(z) or np.iscomplexobj(rhs_):
            return residual_ok(Lm, z.real, rhs_.real) and residual_ok(Lm, z.imag, rhs_.imag)
        return bool((np.abs(Lm @ z - rhs_) <= n * u * (np.abs(Lm) @ np.abs(z))).all())

    sm = hmat.SolveMat(T(L), tri=True, lower=True, chol=True)
    mid_t = sm(vd, chol=False)                                                      # the intermediate of the two-solve form
    mid, z = to_np(mid_t), to_np(sm(vd))
    assert residual_ok(L, mid, v) and residual_ok(L.T, z, mid)
    L00, L10, L11 = L[:n0, :n0], L[n0:, :n0], L[n0:, n0:]
    off = hmat.DenseMat(T(L10))
    for ts in (False, True):
        S = hmat.SolveHierMat(T(L00), T(L11), A10=hmat.DenseMat(T(L10)), lower=True, trans_solve=ts)
        z1_t = S(vd, trans_solve=False)
        z1 = to_np(z1_t)
        # block substitution: each triangular solve by its own residual, the off-diagonal product through the plan
        assert residual_ok(L00, z1[:n0], v[:n0])
        assert residual_ok(L11, z1[n0:], to_np(vd[n0:] - off(z1_t[:n0].contiguous())))
        if not ts:
            assert torch.equal(S(vd), z1_t)
            continue
        # the second half of L L^T z = x through its intermediate z1: backward substitution against the transpose
        z2_t = S.to_transpose()(z1_t, trans_solve=False)
        z2 = to_np(z2_t)
        assert residual_ok(L11.T, z2[n0:], z1[n0:])
        assert residual_ok(L00.T, z2[:n0], to_np(z1_t[:n0] - off(z2_t[n0:].contiguous(), transpose=True)))
        assert torch.equal(S(vd), z2_t)


@pytest.fixture(scope='module')
def tlr():
    return hc.tlr_problem()


def _dist(r, ref):
    return float(np.abs(r - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize('kind', hc.TLR_KINDS)
def test_direction_with_an_hmat_starting_matrix(tlr, kind):
    """the kernel path at most TLR_FACTOR times as far from the float64 golden as the float32 (float64) torch restatement of
    the reference's recursion on the CPU; measured 2026-10-18: see hmat_common.TLR32_RESTATEMENT / TLR32_KERNEL"""
    from bayeslim_amd import hmat, bfgs
    s, y, vec, rho, specs = tlr
    ref = hc.golden()['tlr_' + kind]
    A = hc.dense(specs[kind])
    for dtype in (torch.float32, torch.float64):
        c = lambda a: torch.as_tensor(a).to(dtype)
        Ad = c(A)
        e_rest = _dist(hc.two_loop_torch(c(vec), c(s), c(y), c(rho), lambda q: Ad @ q).double().numpy(), ref)
        H0 = hc.build(specs[kind], hmat, dev(dtype))
        T = dev(dtype)
        r = bfgs.two_loop_recursion(T(vec), list(T(s)), list(T(y)), [float(x) for x in rho], H0=H0)
        e_kern = _dist(to_np(r), ref)
        print('tlr %s %s: restatement %.3e  kernel path %.3e' % (kind, dtype, e_rest, e_kern))
        assert e_kern <= hc.TLR_FACTOR * max(e_rest, hc.U64 if dtype == torch.float64 else 0.0)


def test_lbfgs_with_the_exact_inverse_hessian_converges_sooner():
    from bayeslim_amd import hmat, bfgs
    rng = np.random.default_rng(21)
    N, n0 = 300, 120
    a = rng.normal(size=(n0, n0)) / np.sqrt(n0)
    H1 = a @ a.T + 0.1 * np.eye(n0)
    d2 = rng.uniform(0.1, 10.0, N - n0)
    T = dev(torch.float64)
    hess = torch.block_diag(T(H1), torch.diag(T(d2)))
    x0 = T(rng.normal(size=N))

    def run(H0, update_Hdiag=False):
        p = x0.clone().requires_grad_(True)
        opt = bfgs.LBFGS((p,), H0=H0, max_iter=60, history_size=20, tolerance_grad=1e-9, update_Hdiag=update_Hdiag)
        calls = [0]

        def closure():
            calls[0] += 1
            opt.zero_grad()
            loss = 0.5 * (p @ (hess @ p))
            loss.backward()
            return loss
        opt.step(closure)
        if update_Hdiag and H0 is not None:
            # gamma follows eqn 7.20 with the operator's diagonal as the metric; the operator itself is left alone
            assert opt._gamma != 1.0 and np.isfinite(opt._gamma) and torch.equal(opt._d, H0.diagonal())
            assert torch.allclose(opt._Hdiag, opt._gamma * H0.diagonal(), rtol=1e-15, atol=0)
        return calls[0], float(p.detach().abs().max())

    P = hmat.PartitionedMat({(1, 1): hmat.DenseMat(T(np.linalg.inv(H1))), (2, 2): hmat.DiagMat(T(1 / d2))})
    n_op, x_op = run(P)
    n_id, x_id = run(None)
    # blocks mis-scaled by 3 and 1 / 2: no single step reaches the minimum, so pairs are stored and gamma is rescaled
    P3 = hmat.PartitionedMat({(1, 1): hmat.DenseMat(T(3 * np.linalg.inv(H1))), (2, 2): hmat.DiagMat(T(0.5 / d2))})
    n_up, x_up = run(P3, update_Hdiag=True)
    print('closure calls: exact inverse Hessian %d, mis-scaled blocks with update_Hdiag %d, identity %d' % (n_op, n_up, n_id))
    assert x_op < 1e-8 and n_op < n_id
    assert x_up < 1e-8 and n_up < n_id
