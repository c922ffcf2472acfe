"""
GPU tests of the fused SFB radial transform (csrc/sfb.hip through ops.sfb_radial and sph_harm.SFBModel) against the float64
CPU oracle of tests/sfb_common.py (itself held to the reference's vectors in tests/test_sfb_host.py), never against the
kernel itself.  Tolerances are the project's contract: float64 1e-12 of the maximum, float32 values 1e-5 and gradients 1e-4
of the maximum.  Shapes are the smallest at which a 64 x 32 tile with a 32-deep staged contraction can go wrong.
"""
import copy
import pickle

import numpy as np
import pytest
import torch

from conftest import load_golden
from sfb_common import oracle, oracle_grad, unpack_basis, relmax

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CDT = {torch.float32: torch.complex64, torch.float64: torch.complex128}
DTYPES = {'f64': torch.float64, 'f32': torch.float32}


def tols(prec):
    return (1e-12, 1e-12) if prec == 'f64' else (1e-5, 1e-4)


def to_dev(x, rdt):
    x = torch.as_tensor(x)
    return x.to(device=DEV, dtype=CDT[rdt] if x.is_complex() else rdt)


def run(model, p64, w64, rdt, **kw):
    """forward + backward of Re sum(conj(w) out) on the GPU in precision rdt; records the kernels that ran"""
    from bayeslim_amd import ops
    p = to_dev(p64, rdt).requires_grad_(True)
    prof = []
    ops.PROFILE = prof
    try:
        out = model(p, **kw)
        w = to_dev(w64, rdt)
        ((out * w.conj()).real.sum() if out.is_complex() else (out * w).sum()).backward()
    finally:
        ops.PROFILE = None
    torch.cuda.synchronize()
    assert [k[0] for k in prof] == ['sfb_fwd_kernel', 'sfb_bwd_kernel'], prof
    assert out.dtype == p.dtype and p.grad.dtype == p.dtype
    return out.detach(), p.grad.detach()


# --------------------------------------------------------------------------------------------------------------------
# fixture cases: the reference's own bases
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fixture_cases():
    from bayeslim_amd import sph_harm
    g = load_golden('sfb')
    cases = {}
    for case in ('shell', 'shell_real', 'ball'):
        tag = 'ball' if case == 'ball' else 'shell'
        keys, kln, gln, cols = unpack_basis(g, tag)
        p, w = g[tag + '_params'], g[tag + '_w']
        if case == 'shell_real':
            p, w = p.real.copy(), w.real.copy()
        else:
            gln = {k: v.to(torch.complex128) for k, v in gln.items()}          # complex-typed, as the reference needs them
        Nr, Nlm = len(g[tag + '_r']), len(g[tag + '_l'])
        ref = oracle_grad(p, w, [gln[k].real if gln[k].is_complex() else gln[k] for k in keys], cols, Nr, Nlm)
        sfb = sph_harm.SFBModel()
        sfb.setup_gln(g[tag + '_l'], gln=gln, kln=kln, m=g[tag + '_m'])
        cases[case] = (sfb, p, w, ref)
    return cases


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('case', ['shell', 'shell_real', 'ball'])
def test_fixture_cases(fixture_cases, case, prec):
    sfb, p, w, (ref_out, ref_g) = fixture_cases[case]
    out, gp = run(sfb, p, w, DTYPES[prec])
    assert out.shape == ref_out.shape and out.is_complex() == (case != 'shell_real')
    tv, tg = tols(prec)
    assert relmax(out, ref_out) < tv
    assert relmax(gp, ref_g) < tg


# --------------------------------------------------------------------------------------------------------------------
# tile edges with synthetic tables: random matrices, a hand-made degree array
# --------------------------------------------------------------------------------------------------------------------
NRS = [1, 63, 64, 65, 130]
BATCHES = [(), (3,), (2, 1), (3,), ()]
#        key: (Nk, Nl)   in NON-ASCENDING key order; Nk from {0, 1, 17, 64, 65, 100}, Nl from {1, 31, 32, 33, 70} (and 2)
SYN_KEYS = [(5, 100, 70), (2, 65, 33), (7, 0, 32), (1, 64, 31), (3, 17, 1), (4, 1, 2)]
NO_KEY = 9               # a degree of `l` without a matrix: 4 columns that stay 0


def synthetic_l():
    """173 columns: degree 7 contiguous (32), degree 1 contiguous (31), degree 2 strided (33, every other column),
    degrees 5 (70), 3 (1), 4 (2) and the keyless 9 (4) scattered between and behind them"""
    rng = np.random.default_rng(5)
    pool = rng.permutation([5] * 70 + [NO_KEY] * 4 + [3] * 1 + [4] * 2)
    l = [7] * 32 + [1] * 31
    for i in range(33):
        l += [2, int(pool[i])]
    l += [int(x) for x in pool[33:]]
    return np.asarray(l)


@pytest.fixture(scope='module')
def synthetic():
    """per Nr: (SFBModel, matrices, column lists, l), built once"""
    from bayeslim_amd import sph_harm
    l = synthetic_l()
    built = {}
    for Nr in NRS:
        rng = np.random.default_rng(100 + Nr)
        gln = {key: torch.as_tensor(rng.normal(size=(Nk, Nr))) for key, Nk, _ in SYN_KEYS}
        kln = {key: np.linspace(0.01, 0.1, Nk) for key, Nk, _ in SYN_KEYS}
        sfb = sph_harm.SFBModel()
        sfb.setup_gln(l, gln=gln, kln=kln)
        cols = [np.where(l == key)[0] for key, _, _ in SYN_KEYS]
        assert [len(c) for c in cols] == [Nl for _, _, Nl in SYN_KEYS]
        assert sfb.alm_idx[7] == slice(0, 32, 1) and sfb.alm_idx[2] == slice(63, 129, 2) and isinstance(sfb.alm_idx[5], list)
        assert sfb.Nlmn == sum(Nk * Nl for _, Nk, Nl in SYN_KEYS)
        built[Nr] = (sfb, [gln[key] for key, _, _ in SYN_KEYS], cols, l)
    return built


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('cplx', [True, False], ids=['complex', 'real'])
@pytest.mark.parametrize('iNr', range(len(NRS)), ids=['Nr%d' % n for n in NRS])
def test_tile_edges(synthetic, iNr, cplx, prec):
    Nr, batch = NRS[iNr], BATCHES[iNr]
    sfb, mats, cols, l = synthetic[Nr]
    rng = np.random.default_rng(1000 + 10 * iNr + cplx)
    rnd = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s) if cplx else rng.normal(size=s)
    p, w = rnd(*batch, sfb.Nlmn), rnd(*batch, Nr, len(l))
    ref_out, ref_g = oracle_grad(p, w, mats, cols, Nr, len(l))
    out, gp = run(sfb, p, w, DTYPES[prec])
    assert out.shape == batch + (Nr, len(l)) and gp.shape == batch + (sfb.Nlmn,)
    tv, tg = tols(prec)
    assert relmax(out, ref_out) < tv
    assert relmax(gp, ref_g) < tg
    # columns of the degree with an empty matrix and of the degree without a key are exactly 0
    dead = torch.as_tensor(np.where((l == 7) | (l == NO_KEY))[0], device=DEV)
    assert out.index_select(-1, dead).abs().max().item() == 0.0
    assert torch.isfinite(torch.view_as_real(out) if cplx else out).all()


# --------------------------------------------------------------------------------------------------------------------
# adjoint identity, gradcheck
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cplx', [True, False], ids=['complex', 'real'])
def test_adjoint_identity(synthetic, cplx):
    sfb, mats, cols, l = synthetic[65]
    rng = np.random.default_rng(7)
    rnd = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s) if cplx else rng.normal(size=s)
    p, w = rnd(2, sfb.Nlmn), rnd(2, 65, len(l))
    out, gp = run(sfb, p, w, torch.float64)            # gp = F^H w (F is real: F^H = F^T)
    out, gp = out.cpu().numpy(), gp.cpu().numpy()
    lhs, rhs = np.vdot(w, out), np.vdot(gp, p)
    assert abs(lhs - rhs) < 1e-12 * np.linalg.norm(w) * np.linalg.norm(out)


@pytest.mark.parametrize('cplx', [True, False], ids=['complex', 'real'])
def test_gradcheck_three_degrees(cplx):
    from bayeslim_amd import ops
    rng = np.random.default_rng(11)
    Nr, Nlm = 5, 7
    mats = [torch.as_tensor(rng.normal(size=(Nk, Nr))) for Nk in (3, 1, 2)]
    cols = [np.array([4, 0]), np.array([1, 2, 3]), np.array([6])]             # column 5 belongs to no degree
    plan = ops.SFBPlan(mats, cols, Nr, Nlm, torch.float64, DEV)
    assert not plan.covered and plan.Nlmn == 11
    p = torch.as_tensor(rng.normal(size=(2, 11)) + (1j * rng.normal(size=(2, 11)) if cplx else 0.0), device=DEV)
    p = (p if cplx else p.real).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda q: ops.sfb_radial(q, plan), (p,), eps=1e-6, atol=1e-8, rtol=1e-6)
    ref = oracle(p.detach().cpu(), mats, cols, Nr, Nlm)
    assert relmax(ops.sfb_radial(p, plan), ref) < 1e-12


# --------------------------------------------------------------------------------------------------------------------
# bit identity
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_bit_identity_and_non_contiguous_inputs(synthetic, prec):
    rdt = DTYPES[prec]
    sfb, mats, cols, l = synthetic[130]
    rng = np.random.default_rng(13)
    p = rng.normal(size=(3, sfb.Nlmn)) + 1j * rng.normal(size=(3, sfb.Nlmn))
    w = rng.normal(size=(3, 130, len(l))) + 1j * rng.normal(size=(3, 130, len(l)))
    o1, g1 = run(sfb, p, w, rdt)
    o2, g2 = run(sfb, p, w, rdt)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    # views: every other element of a wider buffer as parameters, a transposed buffer as the upstream gradient
    wide = torch.zeros(3, 2 * sfb.Nlmn, dtype=CDT[rdt], device=DEV)
    wide[:, ::2] = to_dev(p, rdt)
    pv = wide[:, ::2].detach().requires_grad_(True)
    wv = to_dev(w, rdt).permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not pv.is_contiguous() and not wv.is_contiguous()
    ov = sfb(pv)
    ov.backward(wv)                     # d Re sum(conj(w) out): the same upstream gradient as run()
    assert torch.equal(ov.detach(), o1) and torch.equal(pv.grad, g1)


# --------------------------------------------------------------------------------------------------------------------
# object contract
# --------------------------------------------------------------------------------------------------------------------
def test_pickle_deepcopy_push_and_gln_override(fixture_cases):
    from bayeslim_amd import sph_harm
    sfb0, p, w, (ref_out, _) = fixture_cases['shell']
    sfb = copy.deepcopy(sfb0)
    o32, g32 = run(sfb, p, w, torch.float32)
    assert '_plans' in sfb.__dict__
    for clone in (pickle.loads(pickle.dumps(sfb)), copy.deepcopy(sfb)):
        assert '_plans' not in clone.__dict__                   # derived caches do not travel
        oc, gc = run(clone, p, w, torch.float32)
        assert torch.equal(oc, o32) and torch.equal(gc, g32)
    sfb.push(torch.float64)
    assert '_plans' not in sfb.__dict__ and sfb.gln[3].dtype == torch.complex128 and sfb.out_dtype == torch.float64
    o64, _ = run(sfb, p, w, torch.float64)
    assert relmax(o64, ref_out) < 1e-12
    sfb.push(torch.float32)
    assert sfb.gln[3].dtype == torch.complex64
    ob, gb = run(sfb, p, w, torch.float32)
    assert torch.equal(ob, o32) and torch.equal(gb, g32)
    sfb.push(DEV)
    assert sfb.gln[3].is_cuda and str(sfb.device) == DEV
    od, _ = run(sfb, p, w, torch.float32)
    assert torch.equal(od, o32)
    # forward_gln(params, gln=other) == a model set up with other
    rng = np.random.default_rng(17)
    other = {k: torch.as_tensor(rng.normal(size=tuple(v.shape))) for k, v in sfb0.gln.items()}
    o_over, g_over = run(sfb0, p, w, torch.float64, gln=other)
    fresh = sph_harm.SFBModel()
    fresh.setup_gln(sfb0.l, gln=other, kln=sfb0.kln)
    o_new, g_new = run(fresh, p, w, torch.float64)
    assert torch.equal(o_over, o_new) and torch.equal(g_over, g_new)
    keys = list(sfb0.gln.keys())
    assert relmax(o_new, oracle(torch.as_tensor(p), [other[k] for k in keys], unpack_basis(load_golden('sfb'), 'shell')[3],
                                sfb0.Nr, sfb0.Nlm)) < 1e-12
    wrong = dict(other)
    wrong[keys[2]] = wrong[keys[2]][:-1]
    with pytest.raises(ValueError):
        sfb0.forward_gln(to_dev(p, torch.float64), gln=wrong)


def test_make_closure(fixture_cases):
    sfb, p, w, (ref_out, _) = fixture_cases['shell']
    pt = to_dev(p, torch.float64).requires_grad_(True)
    target = to_dev(ref_out, torch.float64)
    closure = sfb.make_closure(pt, lambda a, b: ((a - b).abs() ** 2).sum(), target)
    loss = closure()
    assert loss.item() < 1e-20 * float(ref_out.abs().max()) ** 2 * ref_out.numel() and pt.grad is not None
    loss_r = sfb.make_closure(pt, lambda a, b: ((a - 2 * b) ** 2).sum(), target, real=True)()
    assert abs(loss_r.item() / float((ref_out.real ** 2).sum()) - 1) < 1e-10


# --------------------------------------------------------------------------------------------------------------------
# end to end: t_lmn -> SFBModel -> a_lm(r_nu) -> AlmModel -> pixels -> RIME, against the reference's RIME
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_rime_sfb_mini(prec):
    from bayeslim_amd import sky_model, beam_model, sph_harm, rime_model, utils, telescope_model, ops
    g = load_golden('rime_sfb_mini')
    rdt = DTYPES[prec]
    old = torch.get_default_dtype()
    torch.set_default_dtype(rdt)
    try:
        T = lambda x, dt=None: to_dev(x, dt or rdt)
        freqs = T(g['freqs'])
        antpos = utils.AntposDict(g['ants'].tolist(), torch.as_tensor(g['antvecs'], dtype=torch.float64))
        arr = telescope_model.ArrayModel(antpos, freqs=freqs, cache_s=True, redtol=1.0, device=DEV)
        tel = telescope_model.TelescopeModel((21.42827, -30.72148))
        l, m = g['sky_l'], g['sky_m']
        A = sph_harm.AlmModel(l, m, real_output=True)
        A.device = DEV
        A.setup_Ylm(90.0 - g['dec'], g['ra'], generate=True)
        keys = [int(k) for k in g['sfb_keys']]
        cuts = np.cumsum(g['sfb_nk'])[:-1]
        kln = dict(zip(keys, np.split(g['sfb_kln'], cuts)))
        gln = {k: torch.as_tensor(v) for k, v in zip(keys, np.split(g['sfb_gln'], cuts))}
        sfb = sph_harm.SFBModel()
        sfb.setup_gln(l, gln=gln, kln=kln, m=m)
        assert sfb.Nlmn == g['sky_params'].shape[-1] and sfb.Nr == len(g['freqs'])
        Rs = sky_model.PixelSkyResponse(freqs, spatial_mode='alm', spat_LM=A, LM=sfb, comp_params=False, device=DEV)
        sky = sky_model.PixelSky(T(g['sky_params']), T(np.stack([g['ra'], g['dec']]), torch.float64), float(g['px_area']),
                                 R=Rs, parameter=True, name='sfbsky')
        assert sky.params.is_complex()
        prof = []
        ops.PROFILE = prof
        try:
            with torch.no_grad():
                assert relmax(sky().data, g['sky_map']) < (1e-12 if prec == 'f64' else 3e-6)
        finally:
            ops.PROFILE = None
        assert 'sfb_fwd_kernel' in [k[0] for k in prof]
        tg, pg = T(g['theta_grid'], torch.float64), T(g['phi_grid'], torch.float64)
        b_phi, b_theta = torch.meshgrid(pg, tg, indexing='xy')
        RB = beam_model.YlmResponse(g['beam_l'], g['beam_m'], freqs, pixtype='rect', mode='interpolate', interp_mode='linear',
                                    theta=b_theta.ravel(), phi=b_phi.ravel(), theta_grid=tg, phi_grid=pg, powerbeam=True,
                                    comp_params=True, device=DEV)
        beam = beam_model.PixelBeam(T(g['beam_params']), freqs, R=RB, pol='e', powerbeam=True, fov=180, parameter=False)
        sim_bls = [tuple(b) for b in g['sim_bls']]
        rime = rime_model.RIME(sky, tel, beam, arr, sim_bls, g['times'], freqs)
        Npix = g['zenaz'].shape[-1]
        for t, za in zip(g['times'], g['zenaz']):
            tel.conv_cache[('sfbsky', Npix, float(t))] = torch.as_tensor(za, dtype=torch.float64)
        vis = rime().data
        tv, tgr = (1e-10, 1e-10) if prec == 'f64' else (1e-5, 1e-4)
        assert relmax(vis, g['vis']) < tv
        loss = (vis * T(g['gvis']).conj()).real.sum()
        grad, = torch.autograd.grad(loss, [sky.params])
        assert relmax(grad, g['g_sky_params']) < tgr
    finally:
        torch.set_default_dtype(old)
