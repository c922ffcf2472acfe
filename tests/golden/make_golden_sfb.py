#!/usr/bin/env python3
"""
Golden vectors of the spherical Fourier-Bessel layer (reference sph_harm.py:955-1241, 1851-2145): radial wavenumbers and
transform matrices of a shell and a ball, the index tables of the reference's SFBModel, its transform and gradient for
complex and real parameters, sfb_binning in one and two dimensions, and the reference's RIME on the c3-mini set-up of
make_golden.py with an SFB sky.  TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap and helpers it reuses;
writes tests/golden/sfb.npz and tests/golden/rime_sfb_mini.npz, arrays only, everything float64.

Layout of sfb.npz: per-degree dictionaries are stored as one concatenated array plus the keys and the lengths, e.g.
`shell_kln` (all k_ln, degree after degree), `shell_keys`, `shell_nk`; the matrices as `shell_gln` (sum Nk, Nr), real parts
(the imaginary parts of the reference's complex-typed matrices are exactly 0, asserted here).  params_idx as (start, stop)
rows, alm_idx as the expanded column indices, concatenated, with `shell_nl` columns per key.

Finding (reference, dk_factor=5): the root fit returns NaN for the first k of l = 1, 2; the fixtures use dk_factor=0.5.
Finding (end to end): the reference runs PixelSky(R=PixelSkyResponse(spatial_mode='alm', spat_LM=AlmModel, LM=SFBModel))
in one object once `cosmo` is a placeholder (as for the other fixtures); no hand-chained gradient was needed.

Usage:  python tests/golden/make_golden_sfb.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


def flatten_basis(tag, gln, kln, sfb):
    keys = list(gln.keys())
    for k in keys:
        assert float(gln[k].imag.abs().max()) == 0.0 if gln[k].is_complex() else True
    expand = lambda s, n: np.arange(n)[s] if isinstance(s, slice) else np.asarray(s, dtype=np.int64)
    return {
        tag + '_keys': np.asarray(keys, dtype=np.float64),
        tag + '_nk': np.asarray([len(kln[k]) for k in keys]),
        tag + '_kln': np.concatenate([np.asarray(kln[k], dtype=np.float64) for k in keys]),
        tag + '_gln': np.concatenate([mg.npy(gln[k].real if gln[k].is_complex() else gln[k]) for k in keys]),
        tag + '_params_idx': np.asarray([(sfb.params_idx[k].start, sfb.params_idx[k].stop) for k in keys]),
        tag + '_nl': np.asarray([sfb.alm_shape[k][1] for k in keys]),
        tag + '_alm_idx': np.concatenate([expand(sfb.alm_idx[k], sfb.Nlm) for k in keys]),
        tag + '_Nlmn': np.asarray(sfb.Nlmn), tag + '_k_arr': sfb.k_arr, tag + '_l_arr': np.asarray(sfb.l_arr, dtype=np.float64),
        tag + '_m_arr': np.asarray(sfb.m_arr, dtype=np.float64),
    }


def transform(sfb, p, w):
    p = p.clone().requires_grad_(True)
    out = sfb(p)
    (out * w.conj()).real.sum().backward() if out.is_complex() else (out * w).sum().backward()
    return out.detach(), p.grad.detach()


def gen_sfb(ba):
    sh = ba.sph_harm
    rng = np.random.default_rng(61)
    cn = lambda *s: torch.as_tensor(rng.normal(size=s) + 1j * rng.normal(size=s))
    out = {}

    # shell: 28 columns in m-major order, so the columns of a degree are strided or scattered
    l, m = sh.gen_lm(6, real_field=True)
    r = np.linspace(8800, 9100, 23)
    kw = dict(method='shell', bc_type=2, renorm=True, r_crit=r.min(), r_min=r.min() - 5, r_max=r.max() + 5, kmax=0.12,
              dk_factor=0.5)
    gln, kln = sh.gen_bessel2freq(l, r, dtype=torch.complex128, **kw)
    sfb = sh.SFBModel()
    sfb.setup_gln(l, gln=gln, kln=kln, out_dtype=torch.complex128, m=m)
    assert sfb.Nlmn == 335, sfb.Nlmn
    out.update(flatten_basis('shell', gln, kln, sfb), shell_l=l, shell_m=m, shell_r=r)
    # Dirichlet wavenumbers of the same shell (bc_type=1), degrees 0..6
    out['shell_kln_bc1'] = np.concatenate([sh.sph_bessel_kln(ll, r.min() - 5, r.max() + 5, kmax=0.12, dk_factor=0.5, bc_type=1)
                                           for ll in range(7)])
    out['shell_nk_bc1'] = np.asarray([len(sh.sph_bessel_kln(ll, r.min() - 5, r.max() + 5, kmax=0.12, dk_factor=0.5, bc_type=1))
                                      for ll in range(7)])
    p = cn(2, 1, sfb.Nlmn)
    w = cn(2, 1, sfb.Nr, sfb.Nlm)
    o, g = transform(sfb, p, w)
    out.update(shell_params=p, shell_w=w, shell_out=o, shell_gparams=g)
    # real parameters, real-typed matrices
    gr = {k: v.real.clone() for k, v in gln.items()}
    sr = sh.SFBModel()
    sr.setup_gln(l, gln=gr, kln=kln, out_dtype=torch.float64, m=m)
    pr, wr = p.real.clone(), w.real.clone()
    o, g = transform(sr, pr, wr)
    out.update(shell_out_real=o, shell_gparams_real=g)

    # ball: r_min = 0, lmax 3
    lb, mb = sh.gen_lm(3, real_field=True)
    rb = np.linspace(40.0, 400.0, 17)
    gb, kb = sh.gen_bessel2freq(lb, rb, dtype=torch.complex128, method='ball', bc_type=2, renorm=True, r_min=0.0, r_max=420.0,
                                kmax=0.12, dk_factor=0.5)
    sb = sh.SFBModel()
    sb.setup_gln(lb, gln=gb, kln=kb, out_dtype=torch.complex128, m=mb)
    out.update(flatten_basis('ball', gb, kb, sb), ball_l=lb, ball_m=mb, ball_r=rb)
    pb, wb = cn(3, sb.Nlmn), cn(3, sb.Nr, sb.Nlm)
    o, g = transform(sb, pb, wb)
    out.update(ball_params=pb, ball_w=wb, ball_out=o, ball_gparams=g)

    # sfb_binning on the shell's parameter axis
    kbins = np.linspace(0.01, 0.11, 6)
    lbins = np.array([0.5, 2.5, 4.5])
    var = torch.as_tensor(rng.uniform(0.5, 2.0, size=(2, 1, sfb.Nlmn)))
    wg = torch.as_tensor(rng.uniform(0.5, 2.0, size=(2, 1, sfb.Nlmn)))
    b1, v1 = sh.sfb_binning(p, sfb.k_arr, kbins)
    b1w, v1w = sh.sfb_binning(p, sfb.k_arr, kbins, var=var.clone(), wgts=wg.clone())
    b2, v2 = sh.sfb_binning(p, sfb.k_arr, kbins, l_arr=sfb.l_arr, lbins=lbins)
    b2w, v2w = sh.sfb_binning(p, sfb.k_arr, kbins, var=var.clone(), wgts=wg.clone(), l_arr=sfb.l_arr, lbins=lbins)
    out.update(bin_kbins=kbins, bin_lbins=lbins, bin_var=var, bin_wgts=wg, bin1=b1, bin1_var=v1, bin1w=b1w, bin1w_var=v1w,
               bin2=b2, bin2_var=v2, bin2w=b2w, bin2w_var=v2w)
    mg.save('sfb', **out)


def gen_rime_sfb_mini(ba):
    """the c3-mini set-up of make_golden.gen_rime_c3_mini (array, times, directions, YlmResponse beam) with the sky
    t_lmn -> SFBModel -> a_lm(r_nu) -> AlmModel -> pixels; visibilities and the gradient w.r.t. the complex t_lmn"""
    Nf = 6
    freqs = torch.linspace(120e6, 180e6, Nf)
    times = 2459861.0 + np.arange(2) * 10.0 / 1440
    arr = mg.hex_array(ba, 2, freqs)
    tel = ba.telescope_model.TelescopeModel((21.42827, mg.LAT))
    rng = np.random.default_rng(30)
    Npix = 400
    k = np.arange(Npix) + 0.5
    dec = np.rad2deg(np.arcsin(1 - 2 * k / Npix))
    ra = (k * 137.50776405) % 360.0
    ra_t, dec_t = torch.as_tensor(ra), torch.as_tensor(dec)
    l, m = ba.sph_harm.gen_lm(6)
    colat = 90.0 - dec
    Ysky, _, mult = ba.sph_harm.gen_sph2pix(colat * ba.utils.D2R, ra * ba.utils.D2R, l, m, high_prec=False)
    A = ba.sph_harm.AlmModel(l, m, real_output=True)
    A.setup_Ylm(colat, ra, Ylm=Ysky, alm_mult=mult)
    # one comoving distance per channel (no cosmology: r is an input)
    r = np.linspace(9100.0, 8800.0, Nf)
    gln, kln = ba.sph_harm.gen_bessel2freq(l, r, dtype=torch.complex128, method='shell', bc_type=2, renorm=True, r_crit=r.min(),
                                           r_min=r.min() - 5, r_max=r.max() + 5, kmax=0.12, dk_factor=0.5)
    sfb = ba.sph_harm.SFBModel()
    sfb.setup_gln(l, gln=gln, kln=kln, out_dtype=torch.complex128, m=m)
    t = rng.normal(size=(1, 1, sfb.Nlmn)) + 1j * rng.normal(size=(1, 1, sfb.Nlmn))
    t /= (1.0 + sfb.l_arr)
    sp = torch.as_tensor(t)
    Rs = ba.sky_model.PixelSkyResponse(freqs, spatial_mode='alm', spat_LM=A, LM=sfb, comp_params=False, cosmo=object())
    px_area = 4 * np.pi / Npix
    sky = ba.sky_model.PixelSky(sp.clone(), torch.stack([ra_t, dec_t]), px_area, R=Rs, parameter=True, name='sfbsky')
    bl_, bm_ = ba.sph_harm.gen_lm(4)
    tg = torch.arange(0, 91, 5.0)
    pg = torch.arange(0, 360, 10.0)
    b_phi, b_theta = torch.meshgrid(pg, tg, indexing='xy')
    b_phi, b_theta = b_phi.ravel(), b_theta.ravel()
    Yb, _, bmult = ba.sph_harm.gen_sph2pix(mg.npy(b_theta) * ba.utils.D2R, mg.npy(b_phi) * ba.utils.D2R, bl_, bm_, high_prec=False)
    RB = ba.beam_model.YlmResponse(bl_, bm_, freqs, pixtype='rect', mode='interpolate', interp_mode='linear', theta=b_theta,
                                   phi=b_phi, theta_grid=tg, phi_grid=pg, powerbeam=True, comp_params=True)
    RB.set_Ylm(Yb, (b_theta, b_phi), alm_mult=bmult)
    bp = rng.normal(size=(1, 1, 1, Nf, len(bl_))) + 1j * rng.normal(size=(1, 1, 1, Nf, len(bl_)))
    bp /= (1.0 + bl_) ** 2
    bp[..., 0] += 3.0
    bp[..., bm_ == 0] = bp[..., bm_ == 0].real
    bpr = torch.view_as_real(torch.as_tensor(bp)).clone()
    beam = ba.beam_model.PixelBeam(bpr.clone(), freqs, R=RB, pol='e', powerbeam=True, fov=180, parameter=False)
    sim_bls = arr.get_bls(uniq_bls=False, keep_autos=False)
    rime = ba.rime_model.RIME(sky, tel, beam, arr, sim_bls, times, freqs)
    zenaz = mg.fill_eq2top(tel, sky.name, ra_t, dec_t, times)
    V, gw, grads = mg.run_rime(ba, rime, [sky.params])
    with torch.no_grad():
        skymap = sky().data
    keys = list(gln.keys())
    mg.save('rime_sfb_mini', freqs=freqs, times=times, antvecs=arr.antvecs, ants=np.array(arr.ants), sim_bls=np.array(sim_bls),
            ra=ra, dec=dec, zenaz=zenaz, px_area=np.array(px_area), sky_l=l, sky_m=m, r=r,
            sfb_keys=np.asarray(keys, dtype=np.float64), sfb_nk=np.asarray([len(kln[q]) for q in keys]),
            sfb_kln=np.concatenate([np.asarray(kln[q], dtype=np.float64) for q in keys]),
            sfb_gln=np.concatenate([mg.npy(gln[q].real) for q in keys]), sky_params=sp, sky_map=skymap,
            beam_l=bl_, beam_m=bm_, beam_params=bpr, theta_grid=tg, phi_grid=pg, vis=V, gvis=gw, g_sky_params=grads[0])


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    ba = mg.bootstrap_reference()
    gen_sfb(ba)
    gen_rime_sfb_mini(ba)
