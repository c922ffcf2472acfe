#!/usr/bin/env python3
"""
Golden vectors of the linear-model layer (reference linear_model.py, utils.prep_xarr, linalg.least_squares): gen_poly_A for
every basis, degree, sample set and whitening of lm_common, its options (logx, d0, x0 / dx, qr), gen_fourier_A and its
frequencies, prep_xarr, LinearModel.forward under the cases of lm_common.FWD_CASES, MultiLM over two axes, least_squares
under lm_common.LS_CASES and the out_shape round trip; and a reference RIME.forward + backward whose sky and beam both use
freq_mode='linear' with a polynomial LinearModel.  TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses;
writes tests/golden/lm.npz and tests/golden/rime_lm_mini.npz, arrays only, everything float64 / complex128.

The reference multiplies A and params with matmul / einsum, which refuse operands of different dtypes: where a case pairs a
real with a complex operand, the real one is handed to the reference as a complex tensor of the same values.

Finding (reference): gen_linear_A ends in `.to(dtype)` with dtype = utils._float() when none is passed
(linear_model.py:393-409).  For linear_mode='fourier' that casts the complex matrix of gen_fourier_A to REAL: the
reference returns Re(A) (torch warns that it discards the imaginary part), and so does LinearModel('fourier', x=...).A.
Recorded as four_default (equal to four_None_ortho_A.real, asserted below); the restatement mirrors it, and the complex basis
is reached with an explicit dtype=complex.
Finding (reference): with diag=True a negative dim never matches the axis loop of forward (linear_model.py:137) and the
reshape of A fails; the diag fixtures name their axis with a non-negative dim (the restatement accepts either).
Finding (reference): LinearModel.least_squares casts y to A's dtype first (linear_model.py:193-194), so a complex y with a
real A loses its imaginary part; the complex fixtures pair a complex y with a complex A.

Usage:  python tests/golden/make_golden_lm.py
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import lm_common as lc    # noqa: E402


def gen_lm(ba):
    lm, ut = ba.linear_model, ba.utils
    rng = np.random.default_rng(97)
    out = {}

    # bases
    xs = {'nonuni': torch.as_tensor(np.sort(rng.uniform(0.6, 1.9, 12))), 'uni': torch.linspace(0.6, 1.9, 12)}
    out.update(x_nonuni=xs['nonuni'], x_uni=xs['uni'])
    for basis in lc.BASES:
        for Ndeg in lc.NDEGS:
            for xn in lc.XNAMES:
                for w in (0, 1):
                    out['poly_%s_%d_%s_%d' % (basis, Ndeg, xn, w)] = lm.gen_poly_A(xs[xn], Ndeg, basis=basis, whiten=bool(w))
    for name, kw in lc.POLY_OPTS.items():
        out['poly_opt_%s' % name] = lm.gen_poly_A(xs['nonuni'], 4, basis='legendre', **kw)
    for name, kw in lc.PREP_OPTS.items():
        x, x0, dx = ut.prep_xarr(xs['nonuni'], **kw)
        out['prep_%s_x' % name] = x
        out['prep_%s_x0dx' % name] = np.array([np.nan if v is None else float(v) for v in (x0, dx)])
    for Ndeg, norm in lc.FOURIER:
        A, f = lm.gen_fourier_A(xs['uni'], Ndeg=Ndeg, fft_norm=norm)
        out['four_%s_%s_A' % (Ndeg, norm)], out['four_%s_%s_freqs' % (Ndeg, norm)] = A, f
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out['four_default'] = lm.gen_linear_A('fourier', x=xs['uni'])
        assert not out['four_default'].is_complex()
        assert torch.equal(out['four_default'], out['four_None_ortho_A'].real)
        assert torch.equal(lm.LinearModel('fourier', x=xs['uni']).A, out['four_default'])
    out['four_complex'] = lm.gen_linear_A('fourier', x=xs['uni'], Ndeg=5, dtype=torch.complex128)

    # LinearModel.forward
    out['fwd_xr'], out['fwd_xc'] = lc.rand(rng, lc.FWD_SHAPE, False), lc.rand(rng, lc.FWD_SHAPE, True)
    for K in (2, 3, 4, 5):
        out['fwd_Ar_%d' % K], out['fwd_Ac_%d' % K] = lc.rand(rng, (lc.NS, K), False), lc.rand(rng, (lc.NS, K), True)
        out['fwd_coeff_%d' % K] = torch.as_tensor(rng.uniform(0.5, 2.0, K))
    out['fwd_coeff_full'] = torch.as_tensor(rng.uniform(0.5, 2.0, lc.FWD_SHAPE))
    g = {k: torch.as_tensor(mg.npy(v)) for k, v in out.items()}
    for i, case in enumerate(lc.FWD_CASES):
        x, A, coeff, idx, d = lc.fwd_setup(g, case)
        if not case.get('diag'):
            if x.is_complex() and not A.is_complex():
                A = A.to(torch.complex128)
            if A.is_complex() and not x.is_complex():
                x = x.to(torch.complex128)
        out['fwd_%d' % i] = lc.fwd_model(lm, A, coeff, idx, case, case['dim'])(x)

    # MultiLM over two axes
    out['multi_A2'] = lc.rand(rng, (7, 5), False)
    M = lm.MultiLM([lm.LinearModel('custom', A=g['fwd_Ar_3'], dim=1), lm.LinearModel('custom', A=out['multi_A2'], dim=-1)])
    out['multi_out'] = M(g['fwd_xr'])

    # least_squares
    out['ls_Ar'], out['ls_Ac'] = lc.rand(rng, (lc.NS, 3), False), lc.rand(rng, (lc.NS, 3), True)
    out['ls_yr'], out['ls_yc'] = lc.rand(rng, (2, lc.NS, 5), False), lc.rand(rng, (2, lc.NS, 5), True)
    out['ls_Ninv_vec'] = torch.as_tensor(rng.uniform(0.5, 2.0, lc.NS))
    out['ls_Ninv_full'] = torch.as_tensor(rng.uniform(0.5, 2.0, (2, lc.NS, 5)))
    g = {k: torch.as_tensor(mg.npy(v)) for k, v in out.items()}
    for i, case in enumerate(lc.LS_CASES):
        A, y, Ninv, kw = lc.ls_setup(g, case)
        L = lm.LinearModel('custom', A=A.clone(), dim=1)
        out['ls_%d' % i] = L.least_squares(y.clone(), Ninv=None if Ninv is None else Ninv.clone(), **kw)
    # out_shape round trip: forward flattens (2, NS, 5) to (2, NS * 5), least_squares undoes it
    L = lm.LinearModel('custom', A=g['ls_Ar'].clone(), dim=1, out_reshape=(2, lc.NS * 5), out_shape=(2, lc.NS, 5))
    out['ls_rt_x'] = lc.rand(rng, (2, 3, 5), False)
    out['ls_rt_y'] = L(out['ls_rt_x'])
    out['ls_rt_xhat'] = L.least_squares(out['ls_rt_y'])
    assert (out['ls_rt_xhat'] - out['ls_rt_x']).abs().max() < 1e-12
    mg.save('lm', **out)


def gen_rime_lm_mini(ba):
    """hex-7, 2 times, 6 channels; a 192-pixel PixelSky whose spectrum is a 3-term Legendre polynomial per pixel and a
    rect-grid PixelResponse beam whose spectrum is a 2-term direct polynomial per node, both through LinearModel"""
    Nf = 6
    freqs = torch.linspace(120e6, 180e6, Nf)
    times = 2459861.0 + np.arange(2) * 10.0 / 1440
    arr = mg.hex_array(ba, 2, freqs)
    tel = ba.telescope_model.TelescopeModel((21.42827, mg.LAT))
    rng = np.random.default_rng(61)
    ra, dec = mg.fib_sky(192, cut=False)
    px_area = 4 * np.pi / 192
    sky_LM = ba.linear_model.LinearModel('poly', dim=-2, x=freqs, Ndeg=3, basis='legendre')
    Rs = ba.sky_model.PixelSkyResponse(freqs, freq_mode='linear', freq_LM=sky_LM, cosmo=object())
    sp = torch.as_tensor(rng.normal(size=(1, 1, 3, 192)) * np.array([1.0, 0.3, 0.1])[:, None])
    sky = ba.sky_model.PixelSky(sp.clone(), torch.stack([ra, dec]), px_area, R=Rs, parameter=True, name='lmsky')
    tg, pg = torch.arange(0, 91, 5.0), torch.arange(0, 360, 10.0)
    b_phi, b_theta = torch.meshgrid(pg, tg, indexing='xy')
    b_phi, b_theta = b_phi.ravel(), b_theta.ravel()
    airy = ba.beam_model.airy_disk(b_theta * ba.utils.D2R, b_phi * ba.utils.D2R, 14.0, freqs[Nf // 2:Nf // 2 + 1], square=True)
    beam_LM = ba.linear_model.LinearModel('poly', dim=-2, x=freqs, Ndeg=2, basis='direct')
    R = ba.beam_model.PixelResponse(freqs, 'rect', interp_mode='linear', theta=b_theta, phi=b_phi, theta_grid=tg, phi_grid=pg,
                                    freq_mode='linear', freq_LM=beam_LM, powerbeam=True, realbeam=True)
    a0 = mg.npy(airy).reshape(1, 1, 1, 1, -1)
    bp = torch.as_tensor(np.concatenate([a0, -0.2 * a0 * (1 + 0.1 * rng.normal(size=a0.shape))], axis=3)).clone()
    beam = ba.beam_model.PixelBeam(bp.clone(), freqs, R=R, pol='e', powerbeam=True, fov=180, parameter=True)
    sim_bls = arr.get_bls(uniq_bls=False, keep_autos=False)
    rime = ba.rime_model.RIME(sky, tel, beam, arr, sim_bls, times, freqs)
    zenaz = mg.fill_eq2top(tel, sky.name, ra, dec, times)
    V, gw, grads = mg.run_rime(ba, rime, [sky.params, beam.params])
    mg.save('rime_lm_mini', freqs=freqs, times=times, antvecs=arr.antvecs, ants=np.array(arr.ants), sim_bls=np.array(sim_bls),
            ra=ra, dec=dec, zenaz=zenaz, px_area=np.array(px_area), sky_params=sp, beam_params=bp, theta_grid=tg, phi_grid=pg,
            sky_A=sky_LM.A, beam_A=beam_LM.A, vis=V, gvis=gw, g_sky_params=grads[0], g_beam_params=grads[1])


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    ba = mg.bootstrap_reference()
    gen_lm(ba)
    gen_rime_lm_mini(ba)
