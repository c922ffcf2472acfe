"""
GPU checks of the lightcone sampling (csrc/lcone.hip through ops.lcone_sample and cosmology.cube2lcone / cube2map) against
the float64 restatement of lcone_common, within the bound derived there from the kernel's operation order, and against the
reference's recorded outputs (tests/golden/lcone.npz).
"""
import numpy as np
import pytest
import torch

import lcone_common as lc

pytestmark = pytest.mark.gpu

_REF = {}


def _cubes(prec):
    """the cubes rounded to the working precision (as float64 for the restatement), and their largest magnitude"""
    c = lc.cubes().astype(lc.NPDT[prec])
    return c, c.astype(np.float64), float(np.abs(c).max())


def _restated(prec, order, rinterp, interp, roll, plane):
    """the restatement of a kernel case over ALL directions and radii, computed once and shared: a subset of pixels or a
    leading block of radii is a slice of it"""
    key = (prec, order, rinterp, interp, roll, plane)
    if key not in _REF:
        idx, wgt, S = lc.stencil(lc.SIM_R[order], lc.R, rinterp)
        _REF[key] = lc.restate(_cubes(prec)[1], None if plane else lc.kernel_vectors(), lc.R, idx, wgt, S, lc.SIM_RES, roll, interp)
        _REF[key].setflags(write=False)
    return _REF[key]


def _check(got, want, prec, rinterp, interp, plane, wgt, S, cmax, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == lc.NPDT[prec], what
    if rinterp == 'nearest' and interp == 'nearest':
        assert (got == want.astype(lc.NPDT[prec])).all(), what                       # a pure gather
        return 0.0
    tol = lc.bound(prec, interp, S, plane, wgt, cmax).reshape((-1,) + (1,) * (want.ndim - 1))
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= tol).all(), (what, float((err / tol).max()))
    return float((err / tol).max())


@pytest.mark.parametrize('interp', lc.INTERP)
@pytest.mark.parametrize('rinterp', lc.RINTERP)
@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_kernel_against_the_restatement(prec, rinterp, interp):
    """every roll and both orders of sim_r over all directions and radii; then every Npix of the table (cut from the random
    set, so 1 lane, a wave and a work-group are crossed) with every Nr (a lane's strip of radii is crossed)"""
    from bayeslim_amd import ops
    c, _, cmax = _cubes(prec)
    sims = torch.as_tensor(c).cuda()
    vec = lc.kernel_vectors()
    worst = 0.0
    for order in ('asc', 'desc'):
        idx, wgt, S = lc.stencil(lc.SIM_R[order], lc.R, rinterp)
        for roll in lc.ROLLS:
            want = _restated(prec, order, rinterp, interp, roll, False)
            got = ops.lcone_sample(sims, lc.R, idx, wgt, S, lc.SIM_RES, vec=vec, roll=lc.roll3(roll), interp=interp)
            worst = max(worst, _check(got, want, prec, rinterp, interp, False, wgt, S, cmax, (order, roll)))
    idx, wgt, S = lc.stencil(lc.SIM_R['asc'], lc.R, rinterp)
    want = _restated(prec, 'asc', rinterp, interp, (1, 0, -2), False)
    first = vec.shape[1] - 257                                                        # the random set is the tail
    for k, npix in enumerate(lc.NPIX):
        for nr in sorted({lc.NR[k % len(lc.NR)]} | ({max(lc.NR)} if npix in (1, 257) else set())):
            v = np.ascontiguousarray(vec[:, first:first + npix])
            got = ops.lcone_sample(sims, lc.R[:nr], idx[:nr], wgt[:nr], S, lc.SIM_RES, vec=v, roll=(1, 0, -2), interp=interp)
            worst = max(worst, _check(got, want[:nr, first:first + npix], prec, rinterp, interp, False, wgt[:nr], S, cmax, (npix, nr)))
    print('lcone %s %s x %s: worst error / bound %.3f (K = %d)' % (prec, rinterp, interp, worst, lc.roundings(interp, S, False)))


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_plane_mode_against_the_restatement(prec):
    from bayeslim_amd import ops
    c, _, cmax = _cubes(prec)
    sims = torch.as_tensor(c).cuda()
    for rinterp in lc.RINTERP:
        for interp in lc.INTERP:
            for order in ('asc', 'desc'):
                idx, wgt, S = lc.stencil(lc.SIM_R[order], lc.R, rinterp)
                for roll in lc.ROLLS:
                    want = _restated(prec, order, rinterp, interp, roll, True)
                    got = ops.lcone_sample(sims, lc.R, idx, wgt, S, lc.SIM_RES, vec=None, roll=lc.roll3(roll), interp=interp)
                    assert got.shape == (len(lc.R),) + lc.EXT[:2]
                    _check(got, want, prec, rinterp, interp, True, wgt, S, cmax, (rinterp, interp, order, roll))


def _public(name, sims, pinned=True):
    from bayeslim_amd import cosmology
    G = lc.golden()
    order, ri, si, roll, sphere = lc.fixture_cases(pinned)[name]
    angs = G['angs'] if sphere else None
    if order == 'map':
        return cosmology.cube2map(sims[1], lc.R[2], lc.SIM_RES, angs=angs, roll=roll, interp=si)
    return cosmology.cube2lcone(sims, lc.SIM_R[order], lc.R, lc.SIM_RES, angs=angs, rinterp=ri, interp=si, roll=roll)


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_public_functions_against_the_fixture(prec):
    """cube2lcone / cube2map on the recorded inputs against the reference's recorded outputs: float64 within FACTOR x
    RESTATEMENT of the largest recorded magnitude (bit-equal for 'nearest' x 'nearest'), float32 within the derived bound
    (plus the restatement's own distance from the reference)"""
    G = lc.golden()
    sims = G['sims'].astype(lc.NPDT[prec])
    cmax = float(np.abs(sims).max())
    for name, (order, ri, si, roll, sphere) in lc.fixture_cases().items():
        got, ref = _public(name, sims), G[name]
        assert isinstance(got, np.ndarray) and got.dtype == lc.NPDT[prec] and got.shape == ref.shape, name
        if prec == 'f64':
            if ri == 'nearest' and si == 'nearest':
                assert (got == ref).all(), name
            assert lc.rel_err(got, ref) <= lc.FACTOR * lc.RESTATEMENT, (name, lc.rel_err(got, ref))
            continue
        if order == 'map':
            wgt, S = np.array([[1.0, 0.0, 0.0]]), 1
        else:
            _, wgt, S = lc.stencil(lc.SIM_R[order], lc.R, ri)
        # the reference ran on the unrounded cubes: rounding them to float32 moves the exact result by at most eps/2 W M
        tol = lc.bound(prec, si, S, not sphere, wgt, cmax) + 0.5 * lc.EPS['f32'] * np.abs(wgt[:, :S]).sum(axis=1) * cmax
        tol = tol + lc.FACTOR * lc.RESTATEMENT * np.abs(ref).max()
        err = np.abs(got.astype(np.float64) - ref)
        if order == 'map':
            err = err[None]
        assert (err <= tol.reshape((-1,) + (1,) * (err.ndim - 1))).all(), name


def test_quadratic_is_the_parabola_not_the_references_branch():
    """deviation 1: the public 'quadratic' agrees with the restatement (the Lagrange parabola) and NOT with the reference's
    recorded output"""
    G = lc.golden()
    for name in lc.fixture_cases(False):
        got = _public(name, G['sims'], pinned=False)
        want = lc.restate_fixture(name, pinned=False)
        _, wgt, S = lc.stencil(lc.SIM_R['asc'], lc.R, 'quadratic')
        si = lc.fixture_cases(False)[name][2]
        tol = lc.bound('f64', si, S, False, wgt, float(np.abs(G['sims']).max()))[:, None]
        assert (np.abs(got - want) <= tol).all(), name
        assert lc.rel_err(got, G[name]) > 0.1, name


def test_public_function_behaviour(tmp_path):
    from bayeslim_amd import cosmology
    G = lc.golden()
    sims, angs = G['sims'], G['angs']
    kw = dict(angs=angs, rinterp='linear', interp='linear')
    a = cosmology.cube2lcone(sims, lc.SIM_R['asc'], lc.R, lc.SIM_RES, **kw)
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (len(lc.R), angs.shape[1])
    # a tensor on the GPU gives a tensor on that device, the same bits; twice the same bits
    dev = torch.device('cuda', torch.cuda.current_device())
    t = cosmology.cube2lcone(torch.as_tensor(sims, device=dev), lc.SIM_R['asc'], lc.R, lc.SIM_RES, **kw)
    assert torch.is_tensor(t) and t.device == dev and t.dtype == torch.float64 and (t.cpu().numpy() == a).all()
    t32 = cosmology.cube2lcone(torch.as_tensor(sims, device=dev).float(), torch.as_tensor(lc.SIM_R['asc']), torch.as_tensor(lc.R),
                               lc.SIM_RES, angs=torch.as_tensor(angs), rinterp='linear', interp='linear')
    assert t32.dtype == torch.float32 and t32.device == dev
    assert (cosmology.cube2lcone(sims, lc.SIM_R['asc'], lc.R, lc.SIM_RES, **kw) == a).all()
    # a str is np.load-ed
    path = str(tmp_path / 'boxes.npy')
    np.save(path, sims)
    assert (cosmology.cube2lcone(path, lc.SIM_R['asc'], lc.R, lc.SIM_RES, **kw) == a).all()
    # a roll equals the same call on rolled input, bit for bit; also through a non-contiguous tensor
    for roll in lc.ROLLS[1:]:
        rolled = np.roll(sims, lc.roll3(roll), axis=(1, 2, 3))
        for ang in (angs, None):
            k = dict(kw, angs=ang)
            assert (cosmology.cube2lcone(sims, lc.SIM_R['asc'], lc.R, lc.SIM_RES, roll=roll, **k)
                    == cosmology.cube2lcone(rolled, lc.SIM_R['asc'], lc.R, lc.SIM_RES, **k)).all(), roll
    tt = torch.as_tensor(np.ascontiguousarray(sims.transpose(0, 3, 2, 1)), device=dev).permute(0, 3, 2, 1)
    assert not tt.is_contiguous() and (cosmology.cube2lcone(tt, lc.SIM_R['asc'], lc.R, lc.SIM_RES, **kw).cpu().numpy() == a).all()
    # cube2map is the matching row of cube2lcone: one cube for every r (deviation 2), a scalar r
    for interp in lc.INTERP:
        for ang in (angs, None):
            rows = cosmology.cube2lcone(sims[2], None, lc.R, lc.SIM_RES, angs=ang, interp=interp, roll=3)
            near = cosmology.cube2lcone(sims, lc.SIM_R['asc'], lc.R[3:4], lc.SIM_RES, angs=ang, interp=interp, roll=3)
            for i, r in enumerate(lc.R):
                m = cosmology.cube2map(sims[2], r, lc.SIM_RES, angs=ang, interp=interp, roll=3)
                assert m.shape == rows.shape[1:] and (m == rows[i]).all()
            one = cosmology.cube2lcone(sims[2], None, float(lc.R[3]), lc.SIM_RES, angs=ang, interp=interp, roll=3)
            assert one.shape == (1,) + rows.shape[1:] and (one[0] == rows[3]).all()
            assert (near[0] == cosmology.cube2map(sims[1], lc.R[3], lc.SIM_RES, angs=ang, interp=interp, roll=3)).all()      # the tie: the lower index


def test_offsets_beyond_two_to_the_31():
    """nine float32 cubes of 2^28 voxels: the last cube starts at element 2^31, so an offset held in 32 bits would wrap; the
    stencil reads the first and the last cube at their first and last voxels (positions 0 and -1)"""
    from bayeslim_amd import ops
    sims = torch.zeros((9, 1 << 10, 1 << 9, 1 << 9), dtype=torch.float32, device='cuda')
    assert sims[0].numel() == 1 << 28 and sims.numel() > 1 << 31
    sims[8, -1, -1, -1] = 7.0
    sims[8, 0, 0, 0] = 5.0
    sims[0, -1, -1, -1] = 3.0
    vec = np.array([[-1.0, 0.0], [-1.0, 0.0], [-1.0, 0.0]])
    idx, wgt = np.array([[8, 0, 0], [0, 8, 0]], dtype=np.int32), np.array([[1.0, 0, 0], [0.5, 0.25, 0]])
    got = ops.lcone_sample(sims, np.array([1.0, 1.0]), idx, wgt, 1, 1.0, vec=vec, interp='nearest').cpu().numpy()
    assert got.tolist() == [[7.0, 5.0], [1.5, 0.0]]
    got = ops.lcone_sample(sims, np.array([1.0, 1.0]), idx, wgt, 2, 1.0, vec=vec, interp='linear').cpu().numpy()
    assert got.tolist() == [[7.0, 5.0], [0.5 * 3.0 + 0.25 * 7.0, 0.25 * 5.0]]
