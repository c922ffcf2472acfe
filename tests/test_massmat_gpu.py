"""
The kernels of csrc/massmat.hip and the samplers of bayeslim_amd.massmat on the MI355X, against the float64 restatement of
massmat_common within its derived bound (never a measured tolerance), and bit for bit where the header promises bits: alignment,
NaN above the diagonal, neighbouring blocks, run to run, and nblocks = 0 against rime_hmc_step and the two leaf kernels of nuts.hip.
"""
import numpy as np
import pytest
import torch

import massmat_common as mc
from bayeslim_amd import massmat, nuts, sampler
from bayeslim_amd.paramdict import ParamDict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TD = {'f32': torch.float32, 'f64': torch.float64}
# a block that spans several work-groups of both triangular kernels, and the pairing of first and last strips with an odd count
BIG_N = 5 * max(massmat.UPPER_COLS.values()) * 2 + massmat.LOWER_ROWS + 1


def dev(x, prec):
    return torch.as_tensor(np.asarray(x), dtype=TD[prec], device=DEV).contiguous()


def host(t):
    return t.detach().cpu().double().numpy()


def run_pair(prec, blocks, N, p, g, q, c=None, eps=None, kick=0.05, drift_=0.1, far=None, place=None):
    """project then drift on the GPU for numpy inputs; blocks = [(L, off, nrhs)]; place(L tensor) -> the tensor the table points at"""
    Ls = [(dev(L, prec) if place is None else place(dev(L, prec)), off, nrhs) for L, off, nrhs in blocks]
    table, keep = massmat.make_table(Ls, N, TD[prec], DEV)
    pd, gd, qd = dev(p, prec), dev(g, prec), dev(q, prec)
    cd, ed = (None if c is None else dev(c, prec)), (None if eps is None else dev(eps, prec))
    p_out, z, q_out = torch.empty_like(pd), torch.empty_like(pd), torch.empty_like(pd)
    out = torch.zeros(3, dtype=torch.float64, device=DEV)
    massmat.project(table, pd, gd, ed, cd, kick, p_out, z)
    kw = {} if far is None else dict(p=p_out, q_far=dev(far[0], prec), p_far=dev(far[1], prec))
    massmat.drift(table, z, qd, ed, cd, drift_, q_out, out=out, **kw)
    torch.cuda.synchronize()
    return p_out, z, q_out, out


def reference(prec, blocks, N, p, g, q, c=None, eps=None, kick=0.05, drift_=0.1, far=None):
    u = mc.unit(prec)
    r = lambda x: None if x is None else host(dev(x, prec))
    blocks = [(r(L), off, nrhs) for L, off, nrhs in blocks]
    p, g, q, c, eps = r(p), r(g), r(q), r(c), r(eps)
    p1, dp, z, dz = mc.project(blocks, c, p, g, eps, kick, u)
    q1, dq = mc.drift(blocks, c, z, q, eps, drift_, u, dz)
    K, dK = mc.kinetic(z, u, dz)
    sums = [(K, dK)]
    if far is not None:
        sums += [mc.projection(q1, r(far[0]), r(far[1]), u, dq), mc.projection(q1, r(far[0]), p1, u, dq, dp)]
    return (p1, dp), (z, dz), (q1, dq), sums


def assert_within(got, want):
    val, bound = want
    err = np.abs(host(got) - val)
    assert np.all(err <= bound), 'worst error / bound %.3g at %d' % (np.max(err / np.maximum(bound, 1e-300)), int(np.argmax(err / np.maximum(bound, 1e-300))))


def vectors(N, seed, n=4):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=N) for _ in range(n)]


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('n,nrhs', [(n, 1) for n in mc.ONE_BLOCK_N + (BIG_N,)] + [(65, 2), (BIG_N, 2)])
def test_one_block_against_the_restatement(prec, n, nrhs):
    N = n * nrhs
    blocks = [(mc.factor(n, n), 0, nrhs)]
    p, g, q, qf = vectors(N, n)
    got = run_pair(prec, blocks, N, p, g, q, far=(qf, g))
    want = reference(prec, blocks, N, p, g, q, far=(qf, g))
    for a, b in zip(got[:3], want[:3]):
        assert_within(a, b)
    for k, (val, bound) in enumerate(want[3]):
        assert abs(float(got[3][k]) - val) <= bound, (k, float(got[3][k]), val, bound)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_mixed_layout_against_the_restatement_and_blocks_do_not_see_each_other(prec):
    lay, N = mc.mixed_layout()
    rng = np.random.default_rng(11)
    blocks = [(mc.factor(lay[k][1], 30 + i), lay[k][0], lay[k][2]) for i, k in enumerate(('r', 'w'))]
    c, eps = rng.uniform(0.5, 1.5, N), rng.uniform(0.5, 1.5, N)
    p, g, q, qf = vectors(N, 12)
    got = run_pair(prec, blocks, N, p, g, q, c=c, eps=eps, far=(qf, g))
    want = reference(prec, blocks, N, p, g, q, c=c, eps=eps, far=(qf, g))
    for a, b in zip(got[:3], want[:3]):
        assert_within(a, b)
    for k, (val, bound) in enumerate(want[3]):
        assert abs(float(got[3][k]) - val) <= bound, (k, float(got[3][k]), val, bound)
    # each block alone, at its place: the same bits on its elements
    for L, off, nrhs in blocks:
        alone = run_pair(prec, [(L, off, nrhs)], N, p, g, q, c=c, eps=eps)
        s = slice(off, off + L.shape[0] * nrhs)
        assert torch.equal(alone[1][s], got[1][s]) and torch.equal(alone[2][s], got[2][s])
    # and at another offset with the vector moved along (an odd offset: element accesses of the vectors)
    L, off, nrhs = blocks[0]
    m = L.shape[0]
    mv = lambda v: np.concatenate([np.zeros(3), v[off:off + m], np.zeros(2)])
    moved = run_pair(prec, [(L, 3, 1)], m + 5, mv(p), mv(g), mv(q), eps=mv(eps))
    s = slice(off, off + m)
    assert torch.equal(moved[1][3:3 + m], got[1][s]) and torch.equal(moved[2][3:3 + m], got[2][s])


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('n', [65, 257])
def test_placement_and_the_upper_triangle_do_not_change_a_bit(prec, n):
    blocks = [(mc.factor(n, 40 + n), 0, 1)]
    p, g, q, _ = vectors(n, 41)
    base = run_pair(prec, blocks, n, p, g, q)

    def padded(ld):
        def place(L):
            buf = torch.zeros(n, ld, dtype=L.dtype, device=DEV)
            buf[:, :n] = L
            return buf[:, :n]
        return place

    # n is odd: the baseline (ld = n) takes element loads; ld = n + 3 is a multiple of 16 bytes on an aligned base (16-byte loads),
    # ld = n + 2 is odd again
    assert n % 2 == 1 and (n + 3) % 4 == 0
    aligned_ld, odd_ld = padded(n + 3), padded(n + 2)
    aligned_ld.__name__, odd_ld.__name__ = 'aligned_ld', 'odd_ld'

    def shifted(L):
        buf = torch.zeros(n * n + 1, dtype=L.dtype, device=DEV)
        buf[1:] = L.reshape(-1)
        return buf[1:].view(n, n)

    def nan_above(L):
        return torch.where(torch.ones(n, n, device=DEV).triu(1).bool(), torch.full_like(L, float('nan')), L)

    for place in (aligned_ld, odd_ld, shifted, nan_above):
        got = run_pair(prec, blocks, n, p, g, q, place=place)
        for a, b in zip(got, base):
            assert torch.equal(a, b), place.__name__
        assert not torch.isnan(got[3][0])


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('N', [1, 1001, 2 * sampler.STEP_SPAN[torch.float32] + 5])
def test_no_blocks_is_rime_hmc_step_and_the_nuts_leaf_bit_for_bit(prec, N):
    rng = np.random.default_rng(N)
    p, g, q, c, eps, qf, pf = (dev(rng.normal(size=N), prec) for _ in range(7))
    h = 0.07
    for cc, ee in ((None, None), (c, eps)):
        s = 1.0 if ee is not None else h
        # one stage of hmc_step with the energy
        q1, p1, e1 = q.clone(), p.clone(), torch.zeros(1, dtype=torch.float64, device=DEV)
        sampler.hmc_step(q1, p1, g, ee, cc, 0.5 * s, 1.0 * s, e1)
        p2, z, q2, out = torch.empty_like(p), torch.empty_like(p), torch.empty_like(p), torch.zeros(3, dtype=torch.float64, device=DEV)
        massmat.project(None, p, g, ee, cc, 0.5 * s, p2, z)
        massmat.drift(None, z, q, ee, cc, 1.0 * s, q2, out=out)
        assert torch.equal(p1, p2) and torch.equal(q1, q2) and float(e1[0]) == float(out[0])
        # the leaf of nuts.hip: open, then close against a far state
        qo, po, o3 = torch.empty_like(q), torch.empty_like(p), torch.zeros(3, dtype=torch.float64, device=DEV)
        nuts.leaf_open(q, p, g, qo, po, ee, cc, s)
        assert torch.equal(po, p2) and torch.equal(qo, q2)
        nuts.leaf_close(qo, po, c, ee, cc, s, qf, pf, o3)              # (c as the gradient at the new position)
        p3, o4 = torch.empty_like(p), torch.zeros(3, dtype=torch.float64, device=DEV)
        massmat.project(None, p2, c, ee, cc, 0.5 * s, p3, z)
        massmat.drift(None, z, q2, None, cc, 0.0, None, p=p3, q_far=qf, p_far=pf, out=o4)
        assert torch.equal(po, p3) and o3.tolist() == o4.tolist()


def _problem(prec, seed=21):
    """the mixed ParamDict, its factors and a quadratic potential: (x0, cov_L, diag_mass, potential, flat pieces for the restatement)"""
    lay, N = mc.mixed_layout()
    rng = np.random.default_rng(seed)
    T, CT = TD[prec], {'f32': torch.complex64, 'f64': torch.complex128}[prec]
    Ls = {k: mc.factor(lay[k][1], 50 + i) for i, k in enumerate(('r', 'w'))}
    cd = rng.uniform(0.7, 1.3, lay['d'][1])
    A = {k: mc.spd(lay[k][1], 60 + i) for i, k in enumerate(lay)}
    x0 = {k: rng.normal(size=lay[k][1]) for k in ('d', 'r')}
    x0['w'] = rng.normal(size=lay['w'][1]) + 1j * rng.normal(size=lay['w'][1])
    x = ParamDict({k: torch.as_tensor(v).to(CT if k == 'w' else T).to(DEV) for k, v in x0.items()})
    cov = {'d': dev(cd, prec), 'r': dev(Ls['r'], prec), 'w': dev(Ls['w'], prec)}
    At = {k: dev(v, prec) for k, v in A.items()}

    def potential(q):
        U, grad = 0.0, {}
        for k in q:
            v = q[k].detach()
            Av = torch.complex(At[k] @ v.real, At[k] @ v.imag) if v.is_complex() else At[k] @ v
            grad[k] = Av
            U = U + 0.5 * float((v.conj() * Av).sum().real)
        return U, ParamDict(grad)

    r = lambda a: host(dev(a, prec))
    blocks = [(r(Ls[k]), lay[k][0], lay[k][2]) for k in ('r', 'w')]
    c = np.ones(N)
    c[lay['d'][0]:lay['d'][0] + lay['d'][1]] = r(cd)
    Aflat = [(r(A[k]), lay[k][0], lay[k][2]) for k in lay]
    return x, cov, {'d': True, 'r': False, 'w': False}, potential, (blocks, c, Aflat, N)


def _flat(x, N):
    lay = sampler._Layout(x)
    assert lay.N == N
    return host(lay.pack(x, lay.new()))


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_leapfrog_against_the_restatement_with_launch_count_and_run_to_run_bits(prec):
    x, cov, dm, potential, (blocks, c, Aflat, N) = _problem(prec)
    u, Nstep, eps = mc.unit(prec), 10, 0.05
    rng = np.random.default_rng(5)
    p = ParamDict({k: (torch.as_tensor(rng.normal(size=v.shape) + (1j * rng.normal(size=v.shape) if v.is_complex() else 0)).to(v.dtype).to(DEV))
                   for k, v in x.items()})
    q0, p0 = _flat(x, N), _flat(p, N)
    want = mc.leapfrog(blocks, c, q0, p0, mc.quad_grad(Aflat, u), eps, Nstep, u)
    dUdq = lambda q, Ucache=None: potential(q)[1]
    outs = []
    for _ in range(2):
        q1, p1, states = x.clone(), p.clone(), []
        massmat.leapfrog(q1, p1, dUdq, eps, Nstep, cov_L=cov, diag_mass=dm, states=states)
        outs.append((q1, p1))
        assert len(states) == Nstep + 1
    for k in x:
        assert torch.equal(outs[0][0][k], outs[1][0][k]) and torch.equal(outs[0][1][k], outs[1][1][k])
    qg, pg = _flat(outs[0][0], N), _flat(outs[0][1], N)
    assert np.all(np.abs(qg - want[0]) <= want[1]) and np.all(np.abs(pg - want[2]) <= want[3])
    assert want[1].max() < 1e5 * u                                    # the running bound stays a rounding bound over ten steps


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_hmc_and_nuts_run_on_the_dense_mass(prec):
    x, cov, dm, potential, (blocks, c, Aflat, N) = _problem(prec)
    u = mc.unit(prec)
    np.random.seed(3)
    torch.manual_seed(3)
    s = massmat.HMC(potential, x, 0.05, cov_L=cov, diag_mass=dm, Nstep=6)
    assert s.diag_mass == {'d': True, 'r': False, 'w': False} and s.hess_L['r'] is None and float(s.logdetM) == pytest.approx(
        -2 * np.sum(np.log(c[:37])), rel=1e-5)
    # K of a ParamDict: two launches, against the restatement
    p = s.draw_momentum().clone()
    before = s._traj.launches
    K = float(s.K(p))
    assert s._traj.launches - before == 2
    _, _, z, dz = mc.project(blocks, c, _flat(p, N), None, None, 0.0, u)
    Kw, dK = mc.kinetic(z, u, dz)
    assert abs(K - s._logdetM - Kw) <= dK
    # the draw solves cov_L^T p = p0: L^T p is the unit Gaussian again
    before = s._traj.launches
    accept, prob = s.step()
    assert s._traj.launches - before == 2 * (6 + 1) + 2               # the trajectory and the starting energy
    assert abs(s._last['H_end'] - s._last['H_start']) < 0.5 and 0.0 < float(prob) <= 1.0
    s.sample(3)
    assert len(s.Uchain) == 3 and s.accept_ratio > 0
    # both factors given: the draw multiplies, logdetM counts the dense diagonals
    hess = {'d': 1 / cov['d'], 'r': torch.linalg.inv(cov['r']).T.contiguous(), 'w': torch.linalg.inv(cov['w']).T.contiguous()}
    hess = {k: (torch.linalg.cholesky(v @ v.T) if k != 'd' else v) for k, v in hess.items()}
    s2 = massmat.HMC(potential, x, 0.05, cov_L=cov, hess_L=hess, diag_mass=dm, Nstep=2)
    want = 2 * sum(float(torch.log(hess[k].double().diagonal() if k != 'd' else hess[k].double()).sum()) for k in hess)
    assert float(s2.logdetM) == pytest.approx(want, rel=1e-6)
    s2.step()

    t = massmat.NUTS(potential, x, 0.05, cov_L=cov, diag_mass=dm, max_tree_depth=3)
    evals, launches = t.fn_evals, t.launches
    accept, prob = t.step()
    leaves = t.fn_evals - evals - 1
    assert leaves >= 1 and t.launches - launches == 4 * leaves + 2
    assert abs(t._last['H_end'] - t._last['H_start']) < 0.5
    # a leaf against the restatement: one step from the start in the + direction
    start = t._base_tree.left
    tree = t.build_tree(start, None, 1.0, 0, t._last['H_start'])
    q0, p0 = host(start.q), host(start.p)
    w = mc.leapfrog(blocks, c, q0, p0, mc.quad_grad(Aflat, u), 0.05, 1, u)
    assert np.all(np.abs(host(tree.right.q) - w[0]) <= w[1]) and np.all(np.abs(host(tree.right.p) - w[2]) <= w[3])
    # seeded chains are reproducible bit for bit
    chains = []
    for _ in range(2):
        np.random.seed(9)
        torch.manual_seed(9)
        t = massmat.NUTS(potential, x, 0.05, cov_L=cov, diag_mass=dm, max_tree_depth=3)
        t.sample(3)
        chains.append(np.concatenate([np.asarray(t.chain[k]).view(np.float32 if prec == 'f32' else np.float64).ravel() for k in t.chain]))
    assert np.array_equal(chains[0], chains[1])
