#!/usr/bin/env python3
"""
Golden vectors of a hex-169 (8 antennas on a side, 14 196 baselines): the smallest array of the reference's generator that
the pair cross blocks serve.  TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap and helpers it reuses and whose
`hex128` recipe (gen_rime_mfma_large: 2 channels, 2 times, 600 directions before the declination cut, diffuse signed pixel
sky, rect-linear interpolated PixelBeam) it follows; writes tests/golden/rime_hex169_mini.npz, arrays only.

The visibilities alone are 0.9 MB of float64, so what can be smaller is: the weights of the loss (`gvis` elsewhere) are
integers / 64 in [-2, 2] and are stored as two int8 arrays, gvis = (gvis_re_i8 + 1j * gvis_im_i8) / 64 exactly.

Usage:  python tests/golden/make_golden_hex169.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402


def gen_rime_hex169(ba):
    Nf, Npix, seed = 2, 600, 27
    freqs = torch.linspace(130e6, 170e6, Nf)
    times = 2459861.0 + np.arange(2) * 10.0 / 1440
    rng = np.random.default_rng(seed)
    arr = mg.hex_array(ba, 8, freqs)
    assert len(arr.ants) == 169
    tel = ba.telescope_model.TelescopeModel((21.42827, mg.LAT))
    ra, dec = mg.fib_sky(Npix)
    px_area = 4 * np.pi / Npix
    Rs = ba.sky_model.PixelSkyResponse(freqs, cosmo=object())
    sp = torch.as_tensor(rng.normal(size=(1, 1, Nf, len(ra))))
    sky = ba.sky_model.PixelSky(sp.clone(), torch.stack([ra, dec]), px_area, R=Rs, parameter=True, name='pixsky')
    beam, tg, pg = mg.airy_pixbeam(ba, freqs, parameter=True)
    ants = arr.ants
    sim_bls = [(ants[i], ants[j]) for i in range(len(ants)) for j in range(i + 1, len(ants))]
    rime = ba.rime_model.RIME(sky, tel, beam, arr, sim_bls, times, freqs)
    zenaz = mg.fill_eq2top(tel, sky.name, ra, dec, times)
    V = rime().data
    gre = rng.integers(-128, 128, size=tuple(V.shape)).astype(np.int8)
    gim = rng.integers(-128, 128, size=tuple(V.shape)).astype(np.int8)
    gw = torch.as_tensor((gre.astype(np.float64) + 1j * gim.astype(np.float64)) / 64.0)
    (V * gw.conj()).real.sum().backward()
    mg.save('rime_hex169_mini', freqs=freqs, times=times, antvecs=arr.antvecs, ants=np.array(arr.ants),
            sim_bls=np.array(sim_bls, dtype=np.int16), ra=ra, dec=dec, zenaz=zenaz, px_area=np.array(px_area),
            sky_params=sp, beam_params=beam.params.detach(), theta_grid=tg, phi_grid=pg,
            vis=V.detach(), gvis_re_i8=gre, gvis_im_i8=gim, g_sky_params=sky.params.grad.detach(),
            g_beam_params=beam.params.grad.detach())


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen_rime_hex169(mg.bootstrap_reference())
