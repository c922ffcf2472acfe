"""
massmat without a GPU: the numpy restatement of massmat_common against itself in the working precision (it meets every bound it is
used with), the block-table builder, what the module refuses and in which words, the argument checks of rime_mass_project and
rime_mass_drift (they return before any HIP call), that sampler.HMC and nuts.NUTS still refuse a dense mass, and that the kernels
of csrc/massmat.hip use no scratch memory.
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_asm
import massmat_common as mc
from bayeslim_amd import _lib, hmat, massmat, nuts, sampler
from bayeslim_amd.paramdict import ParamDict

EINVAL, EWORKSPACE = -1, -2
PTR = lambda k: ctypes.c_void_p(4096 * (k + 1))           # distinct non-null dummies 4096 bytes apart; never dereferenced


# ------------------------------------------------------------------------------------------------------- the restatement and its bound
def _mixed_case(seed):
    rng = np.random.default_rng(seed)
    lay, N = mc.mixed_layout()
    blocks = [(mc.factor(lay[k][1], 7 + i), lay[k][0], lay[k][2]) for i, k in enumerate(('r', 'w'))]
    c = np.ones(N)
    c[lay['d'][0]:lay['d'][0] + lay['d'][1]] = rng.uniform(0.5, 1.5, lay['d'][1])
    A = [(mc.spd(m, 20 + i), off, nrhs) for i, (off, m, nrhs) in enumerate(lay.values())]
    q, p = rng.normal(size=N), rng.normal(size=N)
    gap = ~mc.covered([(np.eye(m), off, nrhs) for off, m, nrhs in lay.values()], N)
    q[gap] = p[gap] = 0.0
    return blocks, c, A, q, p, N


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_restatement_in_working_precision_meets_its_own_bound(prec):
    """the same formulas evaluated by numpy IN T (another summation order than the kernels') stay within the derived bound of their
    float64 values: the bound covers any order of the sums"""
    u, T = mc.unit(prec), mc.NP_DTYPE[prec]
    blocks, c, A, q, p, N = _mixed_case(3)
    q, p, c = (x.astype(T).astype(np.float64) for x in (q, p, c))
    blocks = [(L.astype(T).astype(np.float64), off, nrhs) for L, off, nrhs in blocks]
    g, _ = mc.quad_grad(A, u)(q, np.zeros(N))
    g = g.astype(T).astype(np.float64)
    p1, dp, z, dz = mc.project(blocks, c, p, g, None, 0.05, u)
    q1, dq = mc.drift(blocks, c, z, q, None, 0.1, u, dz)
    K, dK = mc.kinetic(z, u, dz)
    # in T
    cT, pT, gT, qT = (x.astype(T) for x in (c, p, g, q))
    pT1 = pT - T(0.05) * gT
    zT = cT * pT1
    yT = cT * zT
    for L, off, nrhs in blocks:
        LT = np.tril(L).astype(T)
        for r in range(nrhs):
            s = slice(off + r, off + L.shape[0] * nrhs, nrhs)
            zT[s] = LT.T @ pT1[s]
    for L, off, nrhs in blocks:
        LT = np.tril(L).astype(T)
        for r in range(nrhs):
            s = slice(off + r, off + L.shape[0] * nrhs, nrhs)
            yT[s] = LT @ zT[s]
    qT1 = qT + T(0.1) * yT
    KT = T(0.5) * np.sum(zT * zT, dtype=T)
    assert np.all(np.abs(pT1 - p1) <= dp) and np.all(np.abs(zT - z) <= dz) and np.all(np.abs(qT1 - q1) <= dq)
    assert abs(float(KT) - K) <= dK
    assert dz.max() < 1e3 * u * 45 and dq.max() < 1e3 * u * 45         # and the bound is a bound of rounding, not a loose tolerance


def test_leapfrog_restatement_conserves_energy_and_is_reversible():
    blocks, c, A, q, p, N = _mixed_case(5)
    u = mc.unit('f64')
    grad = mc.quad_grad(A, u)
    H = lambda q, z: 0.5 * np.sum(q * grad(q, 0 * q)[0]) + 0.5 * np.sum(z * z)
    _, _, z0, _ = mc.project(blocks, c, p, None, None, 0.0, u)
    q1, dq, p1, dp, K, dK = mc.leapfrog(blocks, c, q, p, grad, 0.02, 10, u)
    _, _, z1, _ = mc.project(blocks, c, p1, None, None, 0.0, u)
    assert abs(K - 0.5 * np.sum(z1 * z1)) < 1e-12
    assert abs(H(q1, z1) - H(q, z0)) < 2e-3 * abs(H(q, z0))
    q2, _, p2, _, _, _ = mc.leapfrog(blocks, c, q1, -p1, grad, 0.02, 10, u)
    assert np.abs(q2 - q).max() < 1e-12 and np.abs(p2 + p).max() < 1e-12
    assert dq.max() < 1e-12 and dp.max() < 1e-12


# ------------------------------------------------------------------------------------------------------- the block table
def _x():
    f = torch.float32                                          # explicit: the default dtype is not this file's to assume
    return ParamDict({'a': torch.zeros(3, dtype=f), 'd': torch.zeros(2, 2, dtype=f), 'w': torch.zeros(5, dtype=torch.complex64),
                      'b': torch.zeros(4, dtype=f)})


def test_block_table_offsets_and_nrhs():
    lay = sampler._Layout(_x())
    cov = {'a': torch.eye(3), 'd': torch.ones(2, 2), 'w': hmat.DenseMat(torch.eye(5)), 'b': hmat.TriangMat(torch.eye(4))}
    bt = massmat.BlockTable(lay, cov, {'a': False, 'd': True, 'w': False, 'b': False})
    # 'a' at 0 (3 elements), 'd' at 3 (4), the complex key starts on an even element: 8 (a gap at 7), 'b' at 18
    assert [(e['key'], e['off'], e['n'], e['nrhs'], e['ld']) for e in bt.entries] == [('a', 0, 3, 1, 3), ('w', 8, 5, 2, 5), ('b', 18, 4, 1, 4)]
    assert lay.N == 22 and len(bt) == 3
    c = bt.diagonal()
    assert c.tolist() == [1.0] * 22                            # ones on the dense keys and in the gap
    bt = massmat.BlockTable(lay, dict(cov, d=2 * torch.ones(2, 2)), {'a': False, 'd': True, 'w': False, 'b': False})
    c = bt.diagonal()
    assert c.tolist() == [1.0] * 3 + [2.0] * 4 + [1.0] * 15
    # all diagonal: no blocks, and the builder is sampler's
    bt = massmat.BlockTable(lay, None, True)
    assert bt.entries == [] and bt.diagonal() is None


def test_make_table_validates():
    f = torch.float32
    ok = lambda *b: massmat.make_table(list(b), 20, f, 'cpu')
    assert ok() == (None, [])
    E = torch.eye(4, dtype=f)
    with pytest.raises(ValueError, match='overlap'):
        ok((E, 0, 1), (E, 3, 1))
    with pytest.raises(ValueError, match='overlap'):
        ok((E, 0, 2), (E, 7, 1))
    with pytest.raises(ValueError, match='does not fit'):
        ok((E, 17, 1))
    with pytest.raises(ValueError, match='does not fit'):
        ok((E, -1, 1))
    with pytest.raises(ValueError, match='nrhs'):
        ok((E, 0, 3))
    with pytest.raises(ValueError, match='square'):
        ok((torch.ones(4, 3, dtype=f), 0, 1))
    with pytest.raises(ValueError, match='square'):
        ok((E.double(), 0, 1))
    with pytest.raises(ValueError, match='contiguous'):
        ok((torch.ones(4, 8, dtype=f)[:, ::2], 0, 1))
    with pytest.raises(RuntimeError, match='no CPU implementation'):      # valid blocks: the table itself lives on the GPU
        ok((E, 0, 1), (E, 4, 2))


# ------------------------------------------------------------------------------------------------------- what is refused
def test_refusals_and_their_words():
    x = _x()
    pot = lambda q: (0.0, q)
    dm = {'a': False, 'd': True, 'w': False, 'b': True}
    good = {'a': torch.eye(3), 'd': None, 'w': torch.eye(5), 'b': None}

    def refuses(match, exc=NotImplementedError, **kw):
        args = dict(cov_L=good, diag_mass=dm)
        args.update(kw)
        for cls in (massmat.HMC, massmat.NUTS):
            with pytest.raises(exc, match=match):
                cls(pot, x, 0.1, **args)

    refuses('implicit-solve', cov_L=None, hess_L=good)
    refuses('implicit-solve', cov_L=dict(good, a=None), hess_L=good)
    refuses('SolveMat', cov_L=dict(good, a=hmat.SolveMat(torch.eye(3), tri=True)))
    refuses('SolveMat', cov_L=dict(good, a=hmat.DiagMat(torch.ones(3))))
    refuses('SolveMat', cov_L=dict(good, a=object()))
    refuses('upper-triangular', cov_L=dict(good, a=hmat.TriangMat(torch.eye(3), lower=False)))
    refuses('complex', cov_L=dict(good, w=torch.eye(5, dtype=torch.complex64)))
    refuses(r'shape \(3, 2\)', cov_L=dict(good, a=torch.ones(3, 2)))
    refuses(r'shape \(10, 10\)', cov_L=dict(good, w=torch.eye(10)))          # a complex key takes the (n, n) real factor
    refuses('dict or ParamDict', cov_L=torch.eye(3))
    refuses('pmask', pmask={k: None for k in x})
    refuses('hmat', cov_L=dict(good, d=torch.ones(3)))                        # a diagonal key: sampler's judgement and words
    refuses('no CPU implementation', exc=RuntimeError)                        # judged first, then the device
    for word in ('implicit-solve', 'SolveMat', 'HierMat', 'SolveHierMat', 'SparseMat', 'PartitionedMat', 'complex factor', 'wrong shape',
                 'pmask', 'RecycledHMC', 'StepSize', 'DynamicStepSize', 'no CPU path'):
        assert word in massmat.__doc__, word
    with pytest.raises(NotImplementedError):
        sampler.RecycledHMC()


def test_leapfrog_judges_then_needs_a_gpu():
    q, p = torch.zeros(5), torch.zeros(5)
    f = lambda q, Ucache=None: q
    with pytest.raises(NotImplementedError, match='shape'):
        massmat.leapfrog(q, p, f, 0.1, 3, cov_L=torch.eye(4), diag_mass=False)
    with pytest.raises(NotImplementedError, match='complex'):
        massmat.leapfrog(q, p, f, 0.1, 3, cov_L=torch.eye(5, dtype=torch.complex64), diag_mass=False)
    with pytest.raises(TypeError):
        massmat.leapfrog(ParamDict({'a': q}), p, f, 0.1, 3)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        massmat.leapfrog(q, p, f, 0.1, 3, cov_L=torch.eye(5), diag_mass=False)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        massmat.leapfrog(q, p, f, 0.1, 3)


def test_the_old_entry_points_still_refuse_a_dense_mass():
    x = ParamDict({'a': torch.zeros(4)})
    pot = lambda q: (0.0, q)
    for cls in (sampler.HMC, nuts.NUTS):
        with pytest.raises(NotImplementedError, match='diag_mass=False'):
            cls(pot, x, 0.1, cov_L={'a': torch.eye(4)}, diag_mass=False)
        with pytest.raises(NotImplementedError, match='hmat'):
            cls(pot, x, 0.1, cov_L={'a': torch.eye(4)})
    with pytest.raises(NotImplementedError, match='diag_mass=False'):
        sampler.leapfrog(torch.zeros(4), torch.zeros(4), lambda q, Ucache=None: q, 0.1, 3, cov_L=torch.eye(4), diag_mass=False)
    assert 'massmat' in sampler.__doc__ and 'diag_mass=False' in sampler.__doc__


# ------------------------------------------------------------------------------------------------------- the argument checks
def _project(**bad):
    a = dict(dtype=0, N=100, blocks=PTR(0), nblocks=1, p_in=PTR(1), g=PTR(2), eps=None, c=None, kick=0.5, p_out=PTR(3), z=PTR(4), stream=None)
    a.update(bad)
    return _lib.lib.rime_mass_project(*a.values())


def _drift(**bad):
    a = dict(dtype=0, N=100, blocks=PTR(0), nblocks=1, z=PTR(4), q_in=PTR(5), eps=None, c=None, drift=1.0, q_out=PTR(5), p=PTR(1),
             q_far=PTR(6), p_far=PTR(7), out=ctypes.cast(PTR(8), ctypes.c_void_p), workspace=PTR(9),
             workspace_bytes=_lib.lib.rime_mass_workspace(100), stream=None)
    a.update(bad)
    return _lib.lib.rime_mass_drift(*a.values())


@pytest.mark.parametrize('bad', [dict(dtype=2), dict(N=-1), dict(nblocks=-1), dict(blocks=None), dict(p_in=None), dict(z=None),
                                 dict(g=None), dict(p_out=None), dict(p_out=PTR(1)), dict(p_out=ctypes.c_void_p(4096 * 2 + 396)),
                                 dict(z=PTR(1)), dict(z=PTR(3)), dict(kick=float('nan')), dict(kick=1e-60)],
                         ids=lambda b: '-'.join(b))
def test_project_rejects(bad):
    assert _project(**bad) == EINVAL


@pytest.mark.parametrize('bad,code', [(dict(dtype=7), EINVAL), (dict(N=-1), EINVAL), (dict(nblocks=-2), EINVAL), (dict(blocks=None), EINVAL),
                                      (dict(z=None), EINVAL), (dict(q_in=None), EINVAL), (dict(q_out=None), EINVAL),
                                      (dict(p=None), EINVAL), (dict(q_far=None), EINVAL), (dict(p_far=None, p=None), EINVAL),
                                      (dict(drift=float('nan')), EINVAL), (dict(q_out=PTR(4)), EINVAL),
                                      (dict(workspace=None), EWORKSPACE), (dict(workspace_bytes=8), EWORKSPACE),
                                      (dict(drift=1e-60), EINVAL), (dict(drift=1e-60, workspace=None), EWORKSPACE)],
                         ids=lambda b: '-'.join(b) if isinstance(b, dict) else str(b))
def test_drift_rejects(bad, code):
    assert _drift(**bad) == code


def test_calls_with_nothing_to_do_return_ok_without_a_launch():
    assert _drift(drift=0.0, out=None, p=None, q_far=None, p_far=None, q_in=None, q_out=None) == 0
    assert _lib.lib.rime_mass_workspace(100) == 24 and _lib.lib.rime_mass_workspace(-1) == 0
    assert _lib.lib.rime_mass_workspace(10 ** 7) == _lib.lib.rime_nuts_workspace(10 ** 7)


BOUND = 0x3fffffffffffffff                                  # the largest N the entry points take


@pytest.mark.parametrize('bad', [dict(N=BOUND + 1), dict(N=1 << 35), dict(nblocks=0x7fffffff), dict(kick=-1e-60), dict(kick=0.0, z=PTR(1)),
                                 dict(kick=0.0, z=ctypes.c_void_p(4096 * 2 - 396)), dict(z=ctypes.c_void_p(4096 * 4 + 396)),
                                 dict(kick=0.0, g=None, p_out=None, dtype=7)],
                         ids=lambda b: '-'.join(b))
def test_project_rejects_the_rest(bad):
    """the size bound, a grid beyond 2^31 - 1 work-groups, z on the momentum with and without a kick, z on one element of p_out"""
    assert _project(**bad) == EINVAL


@pytest.mark.parametrize('bad,code', [(dict(N=BOUND + 1), EINVAL), (dict(N=1 << 35), EINVAL), (dict(drift=-1e-60), EINVAL),
                                      (dict(q_out=ctypes.c_void_p(4096 * 6 + 396)), EINVAL),          # q_out on part of q_in, not on it
                                      (dict(q_out=ctypes.c_void_p(4096 * 5 - 396)), EINVAL),          # q_out on the last element of z
                                      (dict(drift=0.0, q_in=None, q_out=None), EINVAL),               # projections of no position
                                      (dict(p=None, q_far=None), EINVAL), (dict(p_far=None), EINVAL), # one or two of the three
                                      (dict(drift=0.0, workspace=None), EWORKSPACE),
                                      (dict(drift=0.0, out=None, dtype=7), EINVAL),                   # nothing to do, but judged first
                                      (dict(drift=0.0, out=None, N=-1), EINVAL), (dict(drift=0.0, out=None, p=None), EINVAL)],
                         ids=lambda b: '-'.join(b) if isinstance(b, dict) else str(b))
def test_drift_rejects_the_rest(bad, code):
    assert _drift(**bad) == code


def test_nothing_to_do_is_ok_only_after_every_check():
    assert _drift(drift=0.0, out=None) == 0 and _drift(drift=0.0, out=None, dtype=1, workspace=None, workspace_bytes=0) == 0
    assert _drift(drift=-0.0, out=None, q_in=None, q_out=None) == 0
    assert _lib.lib.rime_mass_workspace(BOUND + 1) == 0 and _lib.lib.rime_mass_workspace(BOUND) == _lib.lib.rime_nuts_workspace(BOUND) > 0


def test_strip_sizes_match_the_kernels():
    src = open(kernel_asm.os.path.join(kernel_asm.ROOT, 'bayeslim_amd', 'csrc', 'massmat.hip')).read()
    assert 'MASS_ROWS = %d' % massmat.LOWER_ROWS in src and 'CS = 8 * W' in src
    assert massmat.UPPER_COLS == {torch.float32: 32, torch.float64: 16}


def test_kernels_use_no_scratch():
    asm, kernels, sizes = kernel_asm.read('massmat')
    assert len(kernels) == 11 and len(sizes) == len(kernels) and max(sizes) == 0, (kernels, sizes)
    assert 'scratch_load' not in asm and 'scratch_store' not in asm and 'global_atomic' not in asm


# ------------------------------------------------------------------------------------------------------- the golden file
def test_restatement_against_the_reference():
    """tests/golden/massmat.npz (the reference's dense-mass leapfrog and HMC.K, float64) within the restatement's own bound"""
    G, u = mc.golden(), mc.unit('f64')
    w = mc.leapfrog([(G['t_L'], 0, 1)], None, G['t_q0'], G['t_p0'], mc.quad_grad([(G['t_A'], 0, 1)], u), mc.GOLDEN_EPS, mc.GOLDEN_NSTEP, u)
    assert np.all(np.abs(w[0] - G['t_q']) <= w[1]) and np.all(np.abs(w[2] - G['t_p']) <= w[3])
    blocks, c, A_of, q0, p0, N = mc.golden_flat(G)
    assert N == 26 and [b[1:] for b in blocks] == [(7, 1), (16, 2)]
    w = mc.leapfrog(blocks, c, q0, p0, mc.quad_grad(A_of, u), mc.GOLDEN_EPS, mc.GOLDEN_NSTEP, u)
    assert np.all(np.abs(w[0] - mc.golden_pack(G, 'd_q_')) <= w[1]) and np.all(np.abs(w[2] - mc.golden_pack(G, 'd_p_')) <= w[3])
    assert np.abs(w[0] - q0).max() > 0.1                               # and the trajectory went somewhere
    _, _, z, dz = mc.project(blocks, c, p0, None, None, 0.0, u)
    K, dK = mc.kinetic(z, u, dz)
    # the reference derives hess_L = 1 / cov_L on the diagonal key alone: logdetM = -2 sum log c
    assert abs(float(G['logdetM']) + 2 * np.sum(np.log(c[:7]))) < 1e-12
    assert abs(K + float(G['logdetM']) - float(G['K'])) <= dK + 8 * u * abs(float(G['logdetM']))


def test_recorded_chains_are_decisive_in_float32():
    """every recorded Metropolis margin |log u - (H_start - H_end)| and every recorded no-U-turn projection is clear of zero by
    more than the float32 tolerance of a move, so the float32 chains must make the recorded decisions"""
    G = mc.golden()
    tol = mc.chain_tol('f32')
    for tag in ('hmc', 'nuts'):
        Hs, He, u = G[tag + '_H_start'], G[tag + '_H_end'], G[tag + '_u_last']
        margin = np.abs(np.log(u) - np.minimum(Hs - He, 0.0))
        assert np.all(margin > 2 * tol * np.abs(Hs)), (tag, margin, 2 * tol * np.abs(Hs))
        assert np.all(G[tag + '_accept'] == (np.log(u) < Hs - He))
    a = G['nuts_angles']
    a = a[a[:, 2] > 0]                                                 # (a tree of one state has no span: the reference tests 0 < 0)
    assert len(a) >= 6 * 3
    assert np.all(np.abs(a[:, 0]) > tol * a[:, 2]) and np.all(np.abs(a[:, 1]) > tol * a[:, 3]), (np.abs(a[:, :2]) / a[:, 2:]).min()
    assert set(G['nuts_nleaf']) == {7.0, 15.0}                          # trees that turn at depth three and one that reaches four
