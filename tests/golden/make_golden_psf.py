#!/usr/bin/env python3
"""
Golden vectors of the full PSF matrix and of what consumes it (reference imaging.py: VisMapper.make_map / compute_P with
contract=None, the module-level compute_P, deconvolve_map, VisData2MapData):
 (a) the reference's own VisMapper -- hex-19 (171 baselines), Airy PixelBeam with fov 120, 48 map pixels, 2 times whose
     cuts differ, 2 channels, 'A2w' normalisation, supplied icov: make_map(return_P=True, contract=None) -> maps, P, D and
     compute_P(contract=None);
 (b) the module-level compute_P(A, w, D, None) of the first time, with what a restatement needs to reproduce it: baseline
     vectors, the cut pixels' angles, the beam on them, w and D;
 (c) deconvolve_map with pinv False / True on a synthetic well-conditioned P (random symmetric positive definite plus
     the identity);
 (d) VisData2MapData: the flags it derives from a small flag array.
Inputs are recorded next to the outputs.  TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes
tests/golden/psf.npz, arrays only.

Usage:  python tests/golden/make_golden_psf.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg      # noqa: E402


def main():
    torch.set_default_dtype(torch.float64)
    ba = mg.bootstrap_reference()
    imaging = importlib.import_module('bayeslim.imaging')
    rng = np.random.default_rng(47)
    freqs = torch.tensor([125e6, 155e6])
    times = np.array([2459861.0, 2459861.0 + 50.0 / 1440])
    arr = mg.hex_array(ba, 3, freqs)
    tel = ba.telescope_model.TelescopeModel((21.42827, mg.LAT))
    bls = arr.get_bls(uniq_bls=False, keep_autos=False)
    Nbl, Npix, Nt, Nf = len(bls), 48, 2, 2
    ra = mg.lst_of(times[0]) + rng.uniform(-70, 80, Npix)
    dec = mg.LAT + rng.uniform(-65, 65, Npix)
    beam, theta_grid, phi_grid = mg.airy_pixbeam(ba, freqs, parameter=False)
    beam.fov = 120
    data = torch.as_tensor(rng.normal(size=(1, 1, Nbl, Nt, Nf)) + 1j * rng.normal(size=(1, 1, Nbl, Nt, Nf)))
    icov = torch.as_tensor(rng.uniform(0.2, 2.0, size=(1, 1, Nbl, Nt, Nf)))
    vd = ba.dataset.VisData()
    vd.setup_meta(tel, arr.to_antpos())
    vd.setup_data(bls, torch.as_tensor(times), freqs, pol='ee', data=data)
    zenaz = np.stack([np.stack(mg.radec_to_zenaz(ra, dec, mg.lst_of(float(t)), mg.LAT)) for t in times])
    vm = imaging.VisMapper(vd, ra, dec, beam=beam)
    for t, za in zip(times, zenaz):
        vm.telescope.conv_cache[(float(t), Npix)] = torch.as_tensor(za)
    vm.set_normalization('A2w', icov=icov)
    out = dict(freqs=freqs, times=times, antvecs=arr.antvecs, ants=np.array(arr.ants), bls=np.array(bls), ra=ra, dec=dec,
               zenaz=zenaz, data=data, icov=icov, beam_params=beam.params.detach(), theta_grid=theta_grid, phi_grid=phi_grid)
    out['maps'], out['P'] = vm.make_map(return_P=True, contract=None)
    out['D'] = vm.D
    out['P_compute'] = vm.compute_P(contract=None)
    cuts = [vm.build_A(t)[1] for t in times]
    inboth = np.intersect1d(mg.npy(cuts[0]), mg.npy(cuts[1]))
    assert 0 < len(inboth) < min(len(cuts[0]), len(cuts[1])) and len(np.union1d(mg.npy(cuts[0]), mg.npy(cuts[1]))) < Npix
    out['cut0'], out['cut1'] = cuts
    # (b) one time through the module-level function
    A, cut = vm.build_A(times[0])
    w = vm.build_w(0)
    zen, az = torch.as_tensor(zenaz[0][0])[cut], torch.as_tensor(zenaz[0][1])[cut]
    b1 = beam.gen_beam(torch.as_tensor(zenaz[0][0]), torch.as_tensor(zenaz[0][1]))[0][0, 0, 0]
    assert float((A.abs() - b1.abs()).abs().max()) < 1e-12
    D1 = vm.D[:, cut]
    out.update(one_blvecs=vm.blvecs, one_zen=zen, one_az=az, one_beam=b1, one_w=w, one_D=D1,
               one_P=imaging.compute_P(A, w, D1, None))
    # (c) deconvolution
    n = 12
    X = rng.normal(size=(Nf, n, n))
    Pd = torch.as_tensor(X @ X.transpose(0, 2, 1) / n + np.eye(n))
    m = torch.as_tensor(rng.normal(size=(Nf, n)))
    out.update(dec_P=Pd, dec_m=m, dec_diag=imaging.deconvolve_map(m, Pd, pinv=False), dec_pinv=imaging.deconvolve_map(m, Pd, pinv=True))
    # (d) the map container: channel 1 flagged everywhere, channel 2 on some baselines and times only
    fbls, ftimes, ffreqs = bls[:3], torch.as_tensor(times), torch.linspace(120e6, 150e6, 4)
    flags = torch.zeros(1, 1, 3, 2, 4, dtype=torch.bool)
    flags[..., 1] = True
    flags[:, :, :2, :, 2] = True
    flags[:, :, 2, 0, 2] = True
    fvd = ba.dataset.VisData()
    fvd.setup_meta(tel, arr.to_antpos())
    fvd.setup_data(fbls, ftimes, ffreqs, pol='ee', data=torch.zeros(1, 1, 3, 2, 4, dtype=torch.complex128), flags=flags)
    # The reference expands the per-channel flags (Npol, Npol, Nfreqs) with flags.expand(flags.shape + (Npix,)): that
    # aligns the CHANNEL axis with the new pixel axis, so it runs only for Npix == Nfreqs and then returns
    # flags[..., f, p] = channel_flag[p], the transpose of the (Npol, 1, Nfreqs, Npix) its comment states.  Recorded as it
    # is, with Npix = Nfreqs = 4; the tests compare the transpose.
    angs = torch.as_tensor(np.stack([ra[:4], dec[:4]]))
    mdata = torch.as_tensor(rng.normal(size=(1, 1, 4, 4)))
    norm = torch.as_tensor(rng.uniform(1, 2, size=(4, 4)))
    md = imaging.VisData2MapData(fvd, data=mdata, angs=angs, norm=norm, df=torch.full((4,), 1e7), name='dirty')
    assert md.pols == ['ee'] and md.name == 'dirty' and md.flags.shape == (1, 1, 4, 4)
    assert md.flags[0, 0, 0].tolist() == [False, True, False, False]
    out.update(md_bls=np.array(fbls), md_freqs=ffreqs, md_flags_in=flags, md_angs=angs, md_data=mdata, md_norm=norm,
               md_flags=md.flags, md_out_data=md.data, md_out_norm=md.norm)
    mg.save('psf', **out)


if __name__ == '__main__':
    main()
