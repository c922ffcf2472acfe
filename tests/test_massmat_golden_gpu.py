"""
bayeslim_amd.massmat on the MI355X against tests/golden/massmat.npz, recorded from the reference's dense-mass sampler.leapfrog,
HMC.K, HMC and NUTS (tests/golden/make_golden_massmat.py): the leapfrog and K within the running bound of massmat_common, the
chains with momenta supplied through pdist from the recorded draws by their decisions (accept sequence, potential evaluations per
move, i.e. the leaves of the tree) and, in float64, their Hamiltonians and positions within massmat_common.chain_tol.  In float32
only the decisions are compared; tests/test_massmat_host.py checks on the golden file that every recorded Metropolis margin and
every recorded no-U-turn projection is clear of zero by more than the float32 tolerance.  Also: the momentum draw through pdist
against its defining equations, and the FactoredInvHessian.to_dense() -> Cholesky -> massmat.HMC / NUTS round trip.
"""
import numpy as np
import pytest
import torch

import bfgs_dense_common as dc
import massmat_common as mc
from bayeslim_amd import bfgs, massmat, sampler
from bayeslim_amd.paramdict import ParamDict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RT = {'f32': torch.float32, 'f64': torch.float64}
CT = {'f32': torch.complex64, 'f64': torch.complex128}
G = mc.golden()
KEYS = [k for k, _, _ in mc.GOLDEN_KEYS]
KIND = {k: kind for k, kind, _ in mc.GOLDEN_KEYS}


def dev(a, prec):
    a = np.asarray(a)
    return torch.as_tensor(a).to(CT[prec] if np.iscomplexobj(a) else RT[prec]).to(DEV).contiguous()


def setup(prec):
    A = {k: dev(G['d_A_' + k], prec) for k in KEYS}
    cov = {k: dev(G['d_L_' + k], prec) for k in KEYS}
    dm = {k: KIND[k] == 'diag' for k in KEYS}

    def potential(x):
        U, g = 0.0, {}
        for k in x:
            v = x[k].detach()
            g[k] = torch.complex(A[k] @ v.real, A[k] @ v.imag) if v.is_complex() else A[k] @ v
            U = U + 0.5 * float((v.conj() * g[k]).sum().real)
        return U, ParamDict(g)

    x0 = ParamDict({k: dev(G['d_q0_' + k], prec) for k in KEYS})
    return potential, x0, cov, dm


def pdist(prec):
    count = {k: 0 for k in KEYS}

    def dist(k):
        def draw():
            count[k] += 1
            return dev(G['draws_' + k][count[k] - 1], prec)
        return draw
    return {k: dist(k) for k in KEYS}


def test_leapfrog_and_K_against_the_reference_in_float64():
    u = mc.unit('f64')
    # a tensor
    q, p = dev(G['t_q0'], 'f64'), dev(G['t_p0'], 'f64')
    A = dev(G['t_A'], 'f64')
    massmat.leapfrog(q, p, lambda x, Ucache=None: A @ x, mc.GOLDEN_EPS, mc.GOLDEN_NSTEP, cov_L=dev(G['t_L'], 'f64'), diag_mass=False)
    n = mc.GOLDEN_TENSOR_N
    w = mc.leapfrog([(G['t_L'], 0, 1)], None, G['t_q0'], G['t_p0'], mc.quad_grad([(G['t_A'], 0, 1)], u), mc.GOLDEN_EPS, mc.GOLDEN_NSTEP, u)
    assert np.all(np.abs(q.cpu().numpy() - G['t_q']) <= w[1]) and np.all(np.abs(p.cpu().numpy() - G['t_p']) <= w[3])
    # the ParamDict
    potential, x0, cov, dm = setup('f64')
    q, p = x0.clone(), ParamDict({k: dev(G['d_p0_' + k], 'f64') for k in KEYS})
    massmat.leapfrog(q, p, lambda x, Ucache=None: potential(x)[1], mc.GOLDEN_EPS, mc.GOLDEN_NSTEP, cov_L=cov, diag_mass=dm)
    blocks, c, Aflat, q0, p0, N = mc.golden_flat(G)
    w = mc.leapfrog(blocks, c, q0, p0, mc.quad_grad(Aflat, u), mc.GOLDEN_EPS, mc.GOLDEN_NSTEP, u)
    lay = sampler._Layout(q)
    flat = lambda x: lay.pack(x, lay.new()).cpu().numpy()
    gq, gp = mc.golden_pack(G, 'd_q_'), mc.golden_pack(G, 'd_p_')
    assert np.all(np.abs(flat(q) - gq) <= w[1]) and np.all(np.abs(flat(p) - gp) <= w[3])
    # K of the recorded momentum
    s = massmat.HMC(potential, x0, mc.GOLDEN_EPS, cov_L=cov, diag_mass=dm, Nstep=mc.GOLDEN_NSTEP)
    _, _, z, dz = mc.project(blocks, c, p0, None, None, 0.0, u)
    K, dK = mc.kinetic(z, u, dz)
    got = float(s.K(ParamDict({k: dev(G['d_p0_' + k], 'f64') for k in KEYS})))
    assert abs(got - float(G['K'])) <= dK + 8 * u * abs(float(G['logdetM'])) and abs(float(s.logdetM) - float(G['logdetM'])) <= 64 * u


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('tag', ['hmc', 'nuts'])
def test_seeded_chains_make_the_reference_decisions(tag, prec):
    potential, x0, cov, dm = setup(prec)
    np.random.seed(mc.GOLDEN_SEED)
    if tag == 'hmc':
        s = massmat.HMC(potential, x0, mc.GOLDEN_EPS, cov_L=cov, diag_mass=dm, Nstep=mc.GOLDEN_NSTEP, pdist=pdist(prec))
    else:
        s = massmat.NUTS(potential, x0, mc.GOLDEN_EPS, cov_L=cov, diag_mass=dm, max_tree_depth=mc.GOLDEN_DEPTH, pdist=pdist(prec))
    for i in range(mc.GOLDEN_STEPS):
        evals = s.fn_evals
        accept, prob = s.step()
        s._acceptances.append(bool(accept))
        s.append_chain(s.x, U=s._U)
        assert float(bool(accept)) == G[tag + '_accept'][i], i
        assert s.fn_evals - evals - 1 == G[tag + '_nleaf'][i], i
        if prec == 'f64':
            tol = mc.chain_tol(prec) * abs(G[tag + '_H_start'][i])
            print('%s move %d: H_start %.3e  H_end %.3e  tol %.3e' % (tag, i, abs(s._last['H_start'] - G[tag + '_H_start'][i]),
                                                                       abs(s._last['H_end'] - G[tag + '_H_end'][i]), tol))
            assert abs(s._last['H_start'] - G[tag + '_H_start'][i]) <= tol and abs(s._last['H_end'] - G[tag + '_H_end'][i]) <= tol
            assert abs(float(prob) - G[tag + '_prob'][i]) <= 2 * tol
            for k in KEYS:
                want = G['%s_x_%s' % (tag, k)][i]
                assert np.abs(s.x[k].cpu().numpy() - want).max() <= mc.chain_tol(prec) * np.abs(want).max(), (i, k)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_momentum_draw_solves_or_multiplies(prec):
    potential, x0, cov, dm = setup(prec)
    u = mc.unit(prec)
    s = massmat.HMC(potential, x0, mc.GOLDEN_EPS, cov_L=cov, diag_mass=dm, pdist=pdist(prec))
    p = s.draw_momentum()
    for k in KEYS:
        p0 = dev(G['draws_' + k][0], prec).cpu().numpy().astype(np.complex128)
        pk, L = p[k].cpu().numpy().astype(np.complex128), cov[k].cpu().double().numpy()
        if dm[k]:                                                 # p = p0 / c
            assert np.all(np.abs(pk * L - p0) <= 4 * u * np.abs(p0))
        else:                                                     # L^T p = p0: the backward error of a triangular solve (Higham 8.5)
            n = L.shape[0]
            assert np.all(np.abs(L.T @ pk - p0) <= 2 * mc.gamma(n, u) * (np.abs(L).T @ np.abs(pk)) + u * np.abs(p0))
    # both factors: p = hess_L p0 per component
    hess = {k: (1 / cov[k] if dm[k] else torch.linalg.cholesky(torch.linalg.inv(cov[k] @ cov[k].T))) for k in KEYS}
    s = massmat.HMC(potential, x0, mc.GOLDEN_EPS, cov_L=cov, hess_L=hess, diag_mass=dm, pdist=pdist(prec))
    p = s.draw_momentum()
    for k in KEYS:
        p0 = dev(G['draws_' + k][0], prec).cpu().numpy().astype(np.complex128)
        pk, H = p[k].cpu().numpy().astype(np.complex128), hess[k].cpu().double().numpy()
        if dm[k]:
            assert np.all(np.abs(pk - H * p0) <= 4 * u * np.abs(pk))
        else:
            assert np.all(np.abs(pk - np.tril(H) @ p0) <= 2 * mc.gamma(H.shape[0], u) * (np.abs(H) @ np.abs(p0)))


def test_factored_inverse_hessian_round_trip():
    """bfgs.FactoredInvHessian(...).to_dense() -> torch.linalg.cholesky -> massmat.HMC / massmat.NUTS on 'main_params'"""
    g = dc.golden()
    a = dc.factored_args(g, 'rank2')
    args = {k: ([t.to(DEV) for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v.to(DEV) if isinstance(v, torch.Tensor) else v)
            for k, v in a.items()}
    F = bfgs.FactoredInvHessian(**args)
    C = F.to_dense()
    C = 0.5 * (C + C.T)
    n = C.shape[0]
    cov_L = ParamDict({'main_params': torch.linalg.cholesky(C)})
    M = torch.linalg.inv(C)

    def potential(x):
        v = x['main_params'].detach()
        gr = M @ v
        return 0.5 * float(v @ gr), ParamDict({'main_params': gr})

    x0 = ParamDict({'main_params': torch.zeros(n, dtype=C.dtype, device=DEV)})
    np.random.seed(1)
    torch.manual_seed(1)
    for cls, kw in ((massmat.HMC, dict(Nstep=8)), (massmat.NUTS, dict(max_tree_depth=4))):
        s = cls(potential, x0, 0.3, cov_L=cov_L, diag_mass=False, **kw)
        s.sample(4)
        # the mass is the potential's own metric: the trajectory is a rotation at unit frequency, its energy error that of the
        # leapfrog at eps = 0.3: the shadow energy 1/2 p^2 + 1/2 (1 - eps^2 / 4) q^2 is conserved, so |dH| <= eps^2 / 4 H
        assert abs(s._last['H_end'] - s._last['H_start']) <= 0.3 ** 2 / 4 * max(s._last['H_start'], s._last['H_end'], 1.0) + 1e-6
        assert len(s.Uchain) == 4 and np.isfinite(s.Uchain).all() and sum(s._acceptances) >= 1
