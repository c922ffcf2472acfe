"""
CPU-side checks of the operator layer (bayeslim_amd/hmat.py, rime_hmat_apply): the flattening of operator trees into tile
tables and row ranges against hand-written tables, plan invalidation, the rejected calls of the ABI, the CPU-tensor errors, the
deviation list of the module docstring, the half-recurrences of bfgs against compact_coeffs, the refusals of bfgs and the
no-scratch property of the built kernels.
"""
import ctypes
import pickle
import re

import numpy as np
import pytest
import torch

import hmat_common as hc
import lbfgs_common as lc
import kernel_asm


def flatten(op, transpose=False):
    from bayeslim_amd import hmat
    b = hmat._Builder(torch.float64, torch.device('cpu'), require_cuda=False)
    assert hmat._emit(op, transpose, 0, 0, 1.0, b)
    rows = [(t['rows'], t['cols'], t['flags'], t['stage'], t['src_off'], t['dst_off'], t['scale'], t['dst_scratch']) for t in b.tiles]
    return b, rows


def test_flattening_against_hand_written_tables():
    from bayeslim_amd import hmat
    T = lambda *s: torch.zeros(*s, dtype=torch.float64)
    A, B = hmat.DenseMat(T(5, 5)), hmat.DenseMat(T(5, 7))
    S = hmat.SparseMat((7, 7), T(7, 2), Hdiag=T(7), hermitian=True)
    P = hmat.PartitionedMat({(1, 1): A, (1, 2): B, (2, 2): S}, symmetric=True)
    b, rows = flatten(P)
    # column 1: A at (0, 0), B^T at rows 5; column 2: B at (0, 5), then U^T (x -> scratch), U (scratch -> y), Hdiag at (5, 5)
    assert rows == [(5, 5, 0, 0, 0, 0, 1.0, False), (5, 7, 1, 0, 0, 5, 1.0, False), (5, 7, 0, 0, 5, 0, 1.0, False),
                    (7, 2, 1, 0, 5, 0, 1.0, True), (7, 2, 4, 1, 0, 5, 1.0, False), (7, 1, 2, 0, 5, 5, 1.0, False)]
    assert b.scratch == 2 and b.tiles[1]['a'] == b.tiles[2]['a'] == B.H.data_ptr() and b.tiles[2]['ld'] == 7
    ranges, ids, first = hmat.build_index(b.tiles, 12, b.scratch)
    # stage 0: rows 0..11 of y see tiles 0, 1, 2, 5 in table order; the scratch rows come from tile 3; stage 1: tile 4, accumulating
    assert ranges.tolist() == [[0, 0, 12, 0, 4], [1, 0, 2, 4, 1], [2, 0, 12, 5, 1]] and ids.tolist() == [0, 1, 2, 5, 3, 4]
    assert first == [0, 2, 3]
    # the transpose of the same tree: every tile flips, the low-rank pair swaps its roles
    _, rows_t = flatten(P, transpose=True)
    assert rows_t == [(5, 5, 1, 0, 0, 0, 1.0, False), (5, 7, 0, 0, 5, 0, 1.0, False), (5, 7, 1, 0, 0, 5, 1.0, False),
                      (7, 2, 1, 0, 5, 0, 1.0, True), (7, 2, 4, 1, 0, 5, 1.0, False), (7, 1, 2, 0, 5, 5, 1.0, False)]
    # HierMat: the scalar becomes the scale, a scalar DiagMat one repeated value, a ZeroMat no tile, a general low-rank leaf
    # V then U; views keep their leading dimension and base
    big = T(10, 9)
    H = hmat.HierMat(hmat.DenseMat(big[1:4, 2:5]), hmat.DiagMat(torch.tensor([2.0], dtype=torch.float64), 4),
                     A01=hmat.SparseMat((3, 4), T(3, 2), V=T(2, 4)), A10=hmat.ZeroMat((4, 3)), scalar=0.5)
    b, rows = flatten(H)
    assert rows == [(3, 3, 0, 0, 0, 0, 0.5, False), (4, 0, 2, 0, 3, 3, 0.5, False), (2, 4, 0, 0, 3, 0, 1.0, True),
                    (3, 2, 4, 1, 0, 0, 0.5, False)]
    assert b.tiles[0]['ld'] == 9 and b.tiles[0]['a'] == big.data_ptr() + 8 * (9 + 2)
    # more rows than one work-group takes: 600 rows are three ranges, a plain tile into the scratch vector goes 4 rows a range
    b, _ = flatten(hmat.SparseMat((600, 600), T(600, 9), V=T(9, 600)))
    ranges, ids, first = hmat.build_index(b.tiles, 600, b.scratch)
    assert [r[1:3] for r in ranges.tolist()] == [[0, 256], [256, 256], [512, 88], [0, 4], [4, 4], [8, 1], [0, 256], [256, 256], [512, 88]]
    assert first == [0, 6, 9] and [r[4] for r in ranges.tolist()] == [0, 0, 0, 1, 1, 1, 1, 1, 1]
    # an input longer than SPLIT: pieces into scratch segments of their own, unit diagonal tiles that add them, the left factor
    old = hmat.SPLIT
    hmat.SPLIT = 32
    try:
        bs, rows = flatten(hmat.SparseMat((100, 100), T(100, 2), hermitian=True))
    finally:
        hmat.SPLIT = old
    U0 = bs.keep[0].data_ptr()
    assert rows == [(32, 2, 1, 0, 0, 0, 1.0, True), (32, 2, 1, 0, 32, 2, 1.0, True), (32, 2, 1, 0, 64, 4, 1.0, True),
                    (4, 2, 1, 0, 96, 6, 1.0, True)] + [(2, 0, 6, 1, 2 * p, 8, 1.0, True) for p in range(4)] + [(100, 2, 4, 2, 8, 0, 1.0, False)]
    assert [t['a'] - U0 for t in bs.tiles[:4]] == [0, 8 * 64, 8 * 128, 8 * 192] and bs.scratch == 10
    ranges, ids, first = hmat.build_index(bs.tiles, 100, bs.scratch)
    assert ranges.tolist() == [[0, 0, 100, 0, 0], [1, 0, 2, 0, 1], [1, 2, 2, 1, 1], [1, 4, 2, 2, 1], [1, 6, 2, 3, 1], [1, 8, 2, 4, 4],
                               [2, 0, 100, 8, 1]] and ids.tolist() == list(range(9)) and first == [0, 5, 6, 7]
    # not flattenable: OneMat, HadamardMat, SolveMat anywhere in the tree
    for leaf in (hmat.OneMat((5, 5)), hmat.HadamardMat(T(5, 5)), hmat.SolveMat(T(5, 5))):
        bb = hmat._Builder(torch.float64, torch.device('cpu'), require_cuda=False)
        assert not hmat._emit(hmat.MatColumn([A, leaf]), False, 0, 0, 1.0, bb)
    tab = hmat.pack_tiles(b.tiles)
    assert tab.dtype.itemsize == 64 and tab['rows'].tolist() == [9, 600] and tab['flags'].tolist() == [0, 4]


def test_plans_are_dropped():
    from bayeslim_amd import hmat
    T = lambda *s: torch.ones(*s, dtype=torch.float64)

    def dropped(obj, action):
        obj._plans = {'sentinel': 1}
        e = hmat._EPOCH[0]
        res = action(obj)
        return '_plans' not in (obj if res is None else res).__dict__ and hmat._EPOCH[0] > e

    A = hmat.DenseMat(T(3, 3))
    P = hmat.PartitionedMat({(1, 1): hmat.DenseMat(T(3, 3)), (2, 2): hmat.DiagMat(T(2))})
    H = hmat.HierMat(hmat.DenseMat(T(2, 2)), hmat.DiagMat(T(2)))
    for obj in (A, hmat.DiagMat(T(3)), hmat.SparseMat((3, 3), T(3, 1), hermitian=True), hmat.TriangMat(T(3, 3)), P, H,
                hmat.MatRow([hmat.DenseMat(T(2, 2)), hmat.DiagMat(T(2))]), hmat.TransposedMat(hmat.DenseMat(T(2, 3)))):
        assert dropped(obj, lambda o: o.scalar_mul(2.0)), obj
        assert dropped(obj, lambda o: o.push(torch.float32)), obj
        assert dropped(obj, lambda o: pickle.loads(pickle.dumps(o))), obj

        def imul(o):
            o *= 2.0
        assert dropped(obj, imul), obj
    assert A.H.dtype == torch.float32 and float(A.H[0, 0]) == 4.0 and float(H.scalar) == 4.0
    md = hmat.MatDict({'a': A})
    e = hmat._EPOCH[0]
    md['a'] = hmat.DiagMat(T(3))
    assert hmat._EPOCH[0] > e


def test_entry_point_rejects_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)
    sf = (ctypes.c_int * 3)(0, 1, 2)
    bad_sf = (ctypes.c_int * 3)(0, 2, 1)

    def call(dtype=0, tiles=one, ntiles=2, ranges=one, ids=one, first=sf, nstages=2, srows=4, x=one, y=one, nrhs=1, ws=one, nbytes=1 << 20):
        return lib.rime_hmat_apply(dtype, tiles, ntiles, ranges, ids, first, nstages, srows, x, y, nrhs, 1.0, 0, ws, nbytes, None)

    assert call(dtype=2) == -1 and call(dtype=-1) == -1
    assert call(ntiles=-1) == -1 and call(nstages=0) == -1 and call(nstages=9) == -1 and call(nrhs=0) == -1 and call(srows=-1) == -1
    assert call(tiles=None) == -1 and call(ids=None) == -1 and call(ranges=None) == -1 and call(first=None) == -1
    assert call(x=None) == -1 and call(y=None) == -1 and call(first=bad_sf) == -1
    need = lib.rime_hmat_workspace(0, 4, 3)
    assert need == 4 * 3 * 4 and lib.rime_hmat_workspace(1, 4, 3) == 96 and lib.rime_hmat_workspace(2, 4, 3) == 0
    assert lib.rime_hmat_workspace(0, 0, 1) == 0 and lib.rime_hmat_workspace(0, 4, 0) == 0
    assert call(nrhs=3, nbytes=need - 1) == -2 and call(ws=None) == -2
    assert call(nrhs=0, nbytes=0) == -1                                    # the arguments are judged before the workspace


def test_cpu_tensors_and_complex_matrices_raise():
    from bayeslim_amd import hmat
    import bayeslim_amd
    assert bayeslim_amd.hmat is hmat
    T = lambda *s: torch.ones(*s, dtype=torch.float64)
    ops = [hmat.DenseMat(T(3, 3)), hmat.DiagMat(T(3)), hmat.SparseMat((3, 3), T(3, 1), hermitian=True), hmat.TriangMat(T(3, 3)),
           hmat.ZeroMat((3, 3)), hmat.OneMat((3, 3)), hmat.HadamardMat(T(3)), hmat.SolveMat(T(3, 3)),
           hmat.PartitionedMat({(1, 1): hmat.DenseMat(T(3, 3))}), hmat.HierMat(hmat.DenseMat(T(2, 2)), hmat.DiagMat(T(1))),
           hmat.SolveHierMat(T(2, 2), T(1, 1)), hmat.MatRow([hmat.DenseMat(T(3, 3))])]
    for op in ops:
        n = op.shape[-1]
        with pytest.raises(RuntimeError, match='no CPU implementation'):
            op(T(n))
        with pytest.raises(RuntimeError, match='no CPU implementation'):
            op.mat_mat_mul(T(n, 2)) if not isinstance(op, hmat.HadamardMat) else op(T(n))
    b = hmat._Builder(torch.float64, torch.device('cpu'), require_cuda=False)
    with pytest.raises(NotImplementedError, match='complex-valued matrices'):
        hmat._emit(hmat.DenseMat(torch.ones(2, 2, dtype=torch.complex128)), False, 0, 0, 1.0, b)
    with pytest.raises(NotImplementedError):
        hmat.make_hodlr(None, None)


def test_torch_plumbing_agrees_with_the_restatement():
    """to_dense, diagonal and the transposes of every tree against the numpy restatement (CPU tensors, no product)"""
    from bayeslim_amd import hmat
    for name, spec in hc.tree_specs().items():
        op = hc.build(spec, hmat, torch.as_tensor)
        A = hc.dense(spec)
        assert np.allclose(op.to_dense().numpy(), A, rtol=1e-14, atol=1e-14), name
        assert np.allclose(op.to_dense(transpose=True).numpy(), A.T, rtol=1e-14, atol=1e-14), name
        assert np.allclose(op.to_transpose().to_dense().numpy(), A.T, rtol=1e-14, atol=1e-14), name
        assert np.array_equal(hc.dense(hc.transpose_spec(spec)), A.T), name
        if A.shape[0] == A.shape[1] and name != 'col':
            assert np.allclose(op.diagonal().numpy(), np.diagonal(A), rtol=1e-13, atol=1e-14), name
    L = torch.as_tensor(np.tril(np.arange(1.0, 17).reshape(4, 4)))
    tri = hmat.TriangMat(L[torch.tril_indices(4, 4)[0], torch.tril_indices(4, 4)[1]])
    assert torch.equal(tri.to_dense(), L) and torch.equal(tri.diagonal(), L.diagonal())
    s = hmat.MatSum([hmat.DenseMat(L), hmat.DenseMat(L)])
    assert torch.equal(s.to_dense(), 2 * L)


def test_docstring_lists_the_deviations():
    from bayeslim_amd import hmat
    doc = hmat.__doc__
    for word in ('SparseMat.to_dense', 'DiagMat.__call__', 'MatRow.__call__', 'TriangMat from a 1-D', 'TriangMat.diagonal', 'MatSum',
                 'make_hodlr', 'out='):
        assert word in doc, word
    assert len(re.findall(r'^\s+\d+\. ', doc, flags=re.M)) == 11


def test_half_recurrences_agree_with_compact_coeffs():
    from bayeslim_amd import bfgs
    rng = np.random.default_rng(3)
    m, N = 6, 40
    s = rng.normal(size=(m, N))
    y = s * rng.uniform(0.5, 2, N)
    v = rng.normal(size=N)
    SY, YY = s @ y.T, y @ y.T
    a, b = bfgs.compact_coeffs(SY, YY, s @ v, y @ v, 1.0)
    alpha = bfgs.first_loop(SY, s @ v)
    q = v - alpha @ y
    b2 = bfgs.second_loop(SY, y @ q, alpha)
    assert np.array_equal(alpha, a) and np.allclose(b2, b, rtol=1e-12, atol=1e-14)
    r = hc.two_loop_torch(torch.as_tensor(v), torch.as_tensor(s), torch.as_tensor(y), torch.as_tensor(1 / np.diagonal(SY)), lambda q: q)
    assert np.allclose(q + b2 @ s, r.numpy(), rtol=1e-12, atol=1e-14)


def test_bfgs_refusals_and_no_apply_without_an_operator(monkeypatch):
    from bayeslim_amd import bfgs, hmat, _lib
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x = torch.zeros(5, requires_grad=True)
        with pytest.raises(NotImplementedError, match='hmat'):
            lc.host_lbfgs()((x,), H0=torch.eye(5))
        with pytest.raises(NotImplementedError, match='hmat'):
            lc.host_lbfgs()((x,), H0=object())
        calls = []
        monkeypatch.setattr(hmat, '_apply', lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError('hmat used')))
        g = lc.golden()
        icov, x0, H0 = lc.traj_problem(g)
        for h in (None, torch.tensor(0.5), H0):
            p = x0.clone().requires_grad_(True)
            opt = lc.host_lbfgs()((p,), H0=h, max_iter=4)

            def closure():
                opt.zero_grad()
                loss = 0.5 * (p @ (icov @ p))
                loss.backward()
                return loss
            opt.step(closure)
            assert opt.n_iter == 4 and len(opt._s) > 0
        assert calls == []
        # an operator is kept as it is and routed to the operator path
        opt = lc.host_lbfgs()((x,), H0=hmat.DiagMat(torch.ones(5)))
        assert opt._op is opt.H and torch.equal(opt._d, torch.ones(5))
        with pytest.raises(AssertionError, match='hmat used'):
            opt.hvp(torch.ones(5))
    finally:
        torch.set_default_dtype(old)


def test_hmat_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/hmat.hip: no kernel has a private segment"""
    _, kernels, sizes = kernel_asm.read('hmat')
    # 2 precisions x 1, 2, 3, 4 right-hand sides per launch
    assert len(kernels) == 8 and all('hmat_apply_kernel' in k for k in kernels), kernels
    assert len(sizes) == 8 and max(sizes) == 0, sizes
