"""
Host-side checks of the cosmology module (bayeslim_amd/cosmology.py, csrc/lcone.hip, ops.lcone_sample): the float64
restatement against the reference's recorded outputs, the radial stencil tables, the Cosmology class against closed forms
and an independent quadrature, the rejected calls of the C ABI and the build's assembly.  Nothing here launches a kernel.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kernel_asm
import lcone_common as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- restatement and tables
@pytest.mark.parametrize('name', list(lc.fixture_cases()))
def test_restatement_reproduces_the_fixture(name):
    """the restatement the GPU tests compare against gives the reference's recorded outputs: bit-equal for a 'nearest'
    radial and 'nearest' spatial case (a pure gather), within FACTOR x RESTATEMENT otherwise; and the recorded constant is
    the one this fixture gives"""
    order, ri, si, roll, sphere = lc.fixture_cases()[name]
    got, ref = lc.restate_fixture(name), lc.golden()[name]
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float64
    if ri == 'nearest' and si == 'nearest':
        assert (got == ref).all()
    err = lc.rel_err(got, ref)
    assert err <= lc.FACTOR * lc.RESTATEMENT and err <= 1.01 * lc.RESTATEMENT, err


def test_recorded_constant_is_attained():
    worst = max(lc.rel_err(lc.restate_fixture(n), lc.golden()[n]) for n in lc.fixture_cases())
    assert 0.9 * lc.RESTATEMENT <= worst <= 1.01 * lc.RESTATEMENT, worst


def test_fixture_covers_the_edges():
    """the recorded directions hold exact zeros and an integer coordinate, negative coordinates and many wraps"""
    v = lc.unit_vectors(lc.golden()['angs'])
    x = (v[:, :, None] * lc.R) / lc.SIM_RES
    assert (v[0] == 0).any() and (x < 0).any() and np.abs(x).max() > 500 * max(lc.EXT)
    assert (x[2] == 4498.0).any() and (x[2] == -4498.0).any()
    s = lc.special_vectors()
    xs = (s[:, :, None] * lc.R) / lc.SIM_RES
    assert ((xs == np.rint(xs)) & (np.abs(xs) > 30)).any(axis=(1, 2)).all()          # an integer on every axis
    assert (np.floor(xs[2]) % lc.EXT[2] == lc.EXT[2] - 1).sum() >= 2 * len(lc.R)       # the z corner wraps
    assert lc.kernel_vectors().shape[1] > 257 + 192


@pytest.mark.parametrize('order', ['asc', 'desc'])
@pytest.mark.parametrize('rinterp', ['linear', 'quadratic'])
def test_stencil_reproduces_its_cubes_at_their_radii(order, rinterp):
    """node property: cubes that are a function of sim_r sampled through the stencil AT a cube's radius give that cube, and
    the quadratic table reproduces every parabola at any radius (the linear table every straight line)"""
    from bayeslim_amd import cosmology
    sim_r = lc.SIM_R[order]
    idx, wgt, S = cosmology.radial_stencil(sim_r, sim_r, rinterp)
    assert S == lc.STENCIL[rinterp] and idx.dtype == np.int32 and wgt.dtype == np.float64
    for i in range(len(sim_r)):
        assert i in idx[i, :S] and (np.diff(idx[i, :S]) > 0).all()
        w = dict(zip(idx[i, :S].tolist(), wgt[i, :S].tolist()))
        assert w.pop(i) == 1.0 and all(v == 0.0 for v in w.values()), (i, idx[i], wgt[i])
    idx, wgt, S = cosmology.radial_stencil(sim_r, lc.R, rinterp)
    ridx, rwgt, _ = lc.stencil(sim_r, lc.R, rinterp)
    assert (idx == ridx).all() and np.abs(wgt - rwgt).max() <= 1e-12 * np.abs(rwgt).max()
    for deg in range(S):
        got = (wgt[:, :S] * sim_r[idx[:, :S]] ** deg).sum(axis=1)
        assert np.abs(got / lc.R ** deg - 1).max() <= 1e-9, (deg, got)       # cancellation of order (r / dr)^deg eps
    assert (np.abs(wgt).sum(axis=1) > 1.5).any()                              # an r outside sim_r extrapolates


def test_nearest_stencil_and_its_tie():
    from bayeslim_amd import cosmology
    for order in ('asc', 'desc'):
        idx, wgt, S = cosmology.radial_stencil(lc.SIM_R[order], lc.R, 'nearest')
        want = [int(np.argmin(np.abs(r - lc.SIM_R[order]))) for r in lc.R]
        assert S == 1 and idx[:, 0].tolist() == want and (wgt[:, 0] == 1).all() and (wgt[:, 1:] == 0).all()
    assert abs(lc.R[3] - lc.SIM_R['asc'][1]) == abs(lc.R[3] - lc.SIM_R['asc'][2])      # the midway radius is a tie


# ------------------------------------------------------------------------------------------------- Cosmology
def _gl_distance(cosmo, z, order, panels):
    """independent composite Gauss-Legendre quadrature of c / (H0 E) over [0, z] in z itself"""
    x, w = np.polynomial.legendre.leggauss(order)
    edges = np.linspace(0.0, z, panels + 1)
    total = 0.0
    for a, b in zip(edges[:-1], edges[1:]):
        total += 0.5 * (b - a) * (w * 299792.458 / cosmo.H(0.5 * (b - a) * (x + 1) + a)).sum()
    return total


def test_cosmology_closed_forms():
    from bayeslim_amd import cosmology
    c = cosmology.Cosmology()
    assert c._f21 == 1.420405751e9 and c._w21 == 0.211061140542
    assert abs(c.Om0 + c.Ogamma0 + c.Onu0 + c.Ode0 - 1.0) <= 2e-16
    assert 5.3e-5 < c.Ogamma0 < 5.5e-5 and 1.3e-3 < c.Onu0 < 1.5e-3          # photons of 2.725 K; one 0.06 eV neutrino
    assert c.efunc(0.0) == pytest.approx(1.0, abs=1e-15) and c.H(0.0) == pytest.approx(67.7, rel=1e-15)
    assert abs(float(c.nu_relative_density(1e9)) / (0.22710731766 * 3.05) - 1) < 1e-9      # all species relativistic
    f = np.linspace(50e6, 250e6, 41)
    z = c.f2z(f)
    assert np.abs(c.z2f(z) / f - 1).max() <= 4e-16
    want = 299792.458 * (1 + z) ** 2 / (c.H(z) * c._f21)
    assert np.abs(c.dRpara_df(z) / want - 1).max() <= 4e-15                    # to rounding: another order of the same products
    # dr/df = -dRpara_df: central difference with step h, truncation h^2 |r'''| / 6 (r''' from a wider difference)
    h = 1e4
    d1 = (c.f2r(f + h) - c.f2r(f - h)) / (2 * h)
    d3 = (c.f2r(f + 2e6) - 2 * c.f2r(f + 1e6) + 2 * c.f2r(f - 1e6) - c.f2r(f - 2e6)) / (2 * 1e6 ** 3)
    trunc = h ** 2 * np.abs(d3) / 6 + 4 * 2.2e-16 * c.f2r(f) / h
    assert (np.abs(d1 + c.dRpara_df(z)) <= 2 * trunc).all(), np.abs(d1 + c.dRpara_df(z)) / trunc
    assert np.abs(c.X2Y(z) / (c.f2r(f) ** 2 * want) - 1).max() <= 4e-15
    assert np.abs(c.tau_to_kpara(z) * want / (2 * np.pi) - 1).max() <= 4e-15
    assert np.abs(c.bl_to_kperp(z) * c.f2r(f) * (299792458.0 / f) / (2 * np.pi) - 1).max() <= 4e-15
    d = c.comoving_distance(z)
    assert isinstance(d, np.ndarray) and type(d.value) is np.ndarray and (d.value == np.asarray(d)).all()
    assert (c.comoving_transverse_distance(z).value == d.value).all() and (c.dRperp_dtheta(z) == d.value).all()
    assert np.ndim(c.comoving_distance(1.0).value) == 0 and np.ndim(c.f2r(150e6)) == 0
    w = cosmology.gauss1d(np.linspace(-3, 3, 31), scale=0.7, loc=0.2)
    assert w.shape == (1, 31) and abs(w.sum() - 1) < 1e-15 and w.argmax() == 16


def test_distance_against_an_independent_quadrature_and_its_inverse():
    from bayeslim_amd import cosmology
    c = cosmology.Cosmology()
    stated = 1e-13                                                            # comoving_distance's docstring
    for f in (50e6, 100e6, 150e6, 200e6, 250e6):
        z = c.f2z(f)
        a, b = _gl_distance(c, z, 20, 64), _gl_distance(c, z, 32, 128)
        assert abs(a / b - 1) <= 1e-12                                        # the two orders agree with each other
        assert abs(c.f2r(f) / b - 1) <= max(stated, 1e-10), (f, c.f2r(f), b)
    f = np.linspace(50e6, 250e6, 101)
    r = c.f2r(f)
    assert (np.diff(r) < 0).all()
    back = c.r2f(r)
    assert back.shape == f.shape and np.abs(back / f - 1).max() <= 1e-10
    one = c.r2f(float(r[7]))
    assert isinstance(one, float) and abs(one / back[7] - 1) <= 1e-12
    assert np.abs(np.asarray(c.comoving_distance(c.f2z(back))) / r - 1).max() <= 2e-12      # converged in r
    assert c.r2f(0.0) == c._f21
    with pytest.raises(ValueError):
        c.r2f(-1.0)
    other = cosmology.Cosmology(H0=70.0, Om0=0.3)
    assert abs(other.f2r(150e6) / c.f2r(150e6) - 1) > 1e-3                    # the parameters are used


# ------------------------------------------------------------------------------------------------- ABI and Python errors
def _args(**kw):
    one = ctypes.c_void_p(8)          # non-null dummy; never dereferenced on a rejected call
    a = dict(dtype=0, mode=0, interp=1, S=2, sims=one, vec=one, dc=one, cube_idx=one, weight=one,
             cube_idx_host=(ctypes.c_int * 6)(0, 1, 0, 2, 3, 0), sim_res=2.0, rx=0, ry=5, rz=6, Nsim=4, Nx=5, Ny=6, Nz=7,
             Nr=2, Npix=11, out=one, stream=None)
    a.update(kw)
    return list(a.values())


def test_rejected_calls_return_einval_without_a_launch():
    """validation precedes every HIP call, so it runs without a GPU: the pointers handed over are never followed"""
    from bayeslim_amd._lib import lib, SIGNATURES
    assert len(_args()) == len(SIGNATURES['rime_lcone_fwd'][1])
    I = lambda *v: (ctypes.c_int * len(v))(*v)
    bad = [dict(dtype=7), dict(dtype=-1), dict(mode=2), dict(mode=-1), dict(interp=2), dict(interp=-1), dict(S=0), dict(S=4),
           dict(sims=None), dict(vec=None), dict(dc=None), dict(cube_idx=None), dict(weight=None), dict(cube_idx_host=None),
           dict(out=None), dict(Nsim=0), dict(Nx=0), dict(Ny=-1), dict(Nz=0), dict(Nr=0), dict(Npix=0), dict(Npix=-3),
           dict(sim_res=0.0), dict(sim_res=-2.0), dict(sim_res=float('nan')), dict(sim_res=float('inf')),
           dict(rx=-1), dict(rx=5), dict(ry=6), dict(rz=7), dict(rz=-1),
           dict(mode=1, vec=None, Npix=31),                                   # plane: Npix is not Nx Ny
           dict(cube_idx_host=I(0, 4, 0, 2, 3, 0)), dict(cube_idx_host=I(0, 1, 0, -1, 3, 0)),
           dict(S=3, cube_idx_host=I(0, 1, 0, 2, 3, 9)),                      # the third column counts with S = 3
           dict(dtype=7, sims=None), dict(dtype=1, S=0)]
    for kw in bad:
        assert lib.rime_lcone_fwd(*_args(**kw)) == -1, kw


def test_python_level_errors():
    from bayeslim_amd import cosmology, ops
    sims, ang = lc.cubes(), lc.fixture_angs()
    with pytest.raises(ValueError, match='interp'):
        cosmology.cube2lcone(sims, lc.SIM_R['asc'], lc.R, lc.SIM_RES, angs=ang, interp='cubic')
    with pytest.raises(ValueError, match='rinterp'):
        cosmology.cube2lcone(sims, lc.SIM_R['asc'], lc.R, lc.SIM_RES, angs=ang, rinterp='cubic')
    with pytest.raises(ValueError, match='needs 3 cubes'):
        cosmology.cube2lcone(sims[:2], lc.SIM_R['asc'][:2], lc.R, lc.SIM_RES, angs=ang, rinterp='quadratic')
    with pytest.raises(ValueError, match='needs 2 cubes'):
        cosmology.cube2lcone(sims[:1], lc.SIM_R['asc'][:1], lc.R, lc.SIM_RES, angs=ang, rinterp='linear')
    with pytest.raises(ValueError, match='single 3-D cube'):
        cosmology.cube2lcone(sims[0], None, lc.R, lc.SIM_RES, angs=ang, rinterp='linear')
    with pytest.raises(ValueError, match='sim_r has'):
        cosmology.cube2lcone(sims, lc.SIM_R['asc'][:3], lc.R, lc.SIM_RES, angs=ang)
    for bad in (sims.astype(np.float16), sims.astype(np.int32), sims.astype(np.complex64), torch.zeros(2, 3, 3, 3, dtype=torch.bfloat16)):
        with pytest.raises(TypeError, match='float32 and float64'):
            cosmology.cube2lcone(bad, lc.SIM_R['asc'][:len(bad)], lc.R, lc.SIM_RES, angs=ang)
    with pytest.raises(ValueError):
        cosmology.cube2map(sims, 9000.0, lc.SIM_RES, angs=ang)                # four axes
    with pytest.raises(ValueError):
        cosmology.cube2lcone(sims, lc.SIM_R['asc'], lc.R, lc.SIM_RES, angs=ang, roll=(1, 2))
    msg = 'no CPU implementation'
    with pytest.raises(RuntimeError, match=msg):                              # a tensor on the CPU
        cosmology.cube2lcone(torch.as_tensor(sims), lc.SIM_R['asc'], lc.R, lc.SIM_RES, angs=ang)
    with pytest.raises(RuntimeError, match=msg):
        idx, wgt, S = lc.stencil(lc.SIM_R['asc'], lc.R, 'nearest')
        ops.lcone_sample(torch.as_tensor(sims), lc.R, idx, wgt, S, lc.SIM_RES, vec=lc.special_vectors())
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=msg):                          # numpy goes through the GPU: none here
            cosmology.cube2lcone(sims, lc.SIM_R['asc'], lc.R, lc.SIM_RES, angs=ang)


def test_cosmology_is_imported_with_the_package_and_fills_the_callers():
    import bayeslim_amd
    assert bayeslim_amd.cosmology.Cosmology is not None
    src = open(os.path.join(ROOT, 'bayeslim_amd', 'sky_model.py')).read()
    assert 'needs the cosmology module' not in src


# ------------------------------------------------------------------------------------------------- the build
def test_kernels_use_no_scratch():
    """the gfx950 assembly of this build: eight kernels (dtype x sphere / plane x nearest / linear), none with a private
    segment, no atomics, no LDS"""
    asm, kernels, sizes = kernel_asm.read('lcone')
    assert len(kernels) == 8 and all('lcone_fwd_kernel' in k for k in kernels), kernels
    assert sizes == [0] * 8, sizes
    assert not re.findall(r'^\s*scratch_(?:load|store)', asm, flags=re.M)
    assert 'atomic' not in asm and not re.findall(r'^\s*ds_', asm, flags=re.M)
    assert re.findall(r'^\s*v_fma_f64', asm, flags=re.M) and re.findall(r'^\s*v_(?:fma|fmac)_f32', asm, flags=re.M)


def test_layout_constants_match_the_source():
    src = open(os.path.join(ROOT, 'bayeslim_amd', 'csrc', 'lcone.hip')).read()
    assert re.search(r'LC_THREADS = %d, LC_RSTRIP = %d\b' % (lc.LC_THREADS, lc.LC_RSTRIP), src)
    assert max(lc.NR) > lc.LC_RSTRIP > min(lc.NR) and max(lc.NPIX) > lc.LC_THREADS          # strips and work-groups are crossed
    assert [lc.roundings(i, s, p) for i, s, p in (('nearest', 1, False), ('linear', 3, False), ('linear', 2, True))] == [2, 16, 7]
