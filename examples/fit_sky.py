"""
End-to-end use of the drop-in modules the way the reference's notebooks drive them: simulate visibilities of a
HERA-37 array over a diffuse pixel sky with an Airy beam, add noise, then recover the sky by minimising the
(negative log) posterior with bfgs.LBFGS through optim.LogProb -- forward model, chi-square and backward all on
the HIP kernels.  usage: python examples/fit_sky.py [iterations]
"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bayeslim_amd import utils, telescope_model, beam_model, sky_model, rime_model, optim, dataset, bfgs


def build(dev, Nf=8, Npix=768, Nt=4, seed=0):
    rng = np.random.default_rng(seed)
    freqs = torch.linspace(120e6, 180e6, Nf, device=dev)
    times = 2459861.0 + np.arange(Nt) * 10.0 / 1440
    ants, vecs = utils._make_hex(4, D=14.6)
    arr = telescope_model.ArrayModel(utils.AntposDict(ants, torch.as_tensor(vecs)), freqs=freqs, device=dev)
    tel = telescope_model.TelescopeModel((21.42827, -30.72148))
    k = np.arange(Npix) + 0.5                                      # Fibonacci-lattice sky directions
    dec = np.rad2deg(np.arcsin(1 - 2 * k / Npix))
    lst = float(telescope_model.JD2LST(times[0], 21.42827))
    ra = (k * 137.50776405 + lst) % 360.0
    truth = torch.as_tensor(np.abs(rng.normal(size=(1, 1, Nf, Npix))) + 0.5, dtype=torch.float32, device=dev)
    angs = torch.as_tensor(np.stack([ra, dec]), device=dev)
    sky = sky_model.PixelSky(truth.clone(), angs, 4 * np.pi / Npix, R=sky_model.PixelSkyResponse(freqs, device=dev),
                             parameter=True, name='sky')
    beam = beam_model.PixelBeam(torch.ones(1, 1, 1, 1, 1, device=dev) * 14.0, freqs, R=beam_model.AiryResponse(powerbeam=True),
                                pol='e', powerbeam=True, fov=180, parameter=False)
    bls = arr.get_bls(uniq_bls=False, keep_autos=False)
    rime = rime_model.RIME(sky, tel, beam, arr, bls, times, freqs)
    for t in times:
        zen, az = telescope_model.eq2top((21.42827, -30.72148), t, ra, dec)
        tel.conv_cache[('sky', Npix, float(t))] = torch.as_tensor(np.stack([zen, az]))
    return rime, sky, truth, bls, times, freqs


def main(niter=8, dev=None, verbose=True):
    dev = dev or torch.device('cuda:0')
    rime, sky, truth, bls, times, freqs = build(dev)
    model = utils.Sequential(dict(rime=rime))
    with torch.no_grad():
        vis = model().data
    gen = torch.Generator(device='cpu').manual_seed(1)
    sig = 0.02 * float(vis.abs().mean())
    noise = torch.complex(torch.randn(vis.shape, generator=gen), torch.randn(vis.shape, generator=gen)).to(dev) * sig
    target = dataset.VisData()
    target.setup_data(bls, torch.as_tensor(times), freqs, pol='ee', data=vis + noise,
                      icov=torch.full(vis.shape, 1 / sig ** 2, device=dev))
    with torch.no_grad():
        sky.params.mul_(0.0).add_(1.0)                              # start from a flat sky
    sky.set_priors(priors_inp_params=[optim.LogGaussPrior(torch.ones((), device=dev), torch.full((), 25.0, device=dev),
                                                          density=False)])
    prob = optim.LogProb(model, dataset.Dataset([target]), device=dev)
    prob.set_main_params(['rime.sky.params'])
    opt = bfgs.LBFGS([prob.main_params], lr=1.0, max_iter=4, history_size=10, line_search_fn='strong_wolfe')
    losses = []
    for it in range(niter):
        # the loss at the start of the step, as torch.optim.LBFGS reports it (bfgs.LBFGS.step returns the loss at its end)
        losses.append(float(prob.closure()) if opt._loss is None else opt._loss)
        opt.step(prob.closure)
        if verbose:
            print('iteration %2d: -log posterior %.6g' % (it, losses[-1]), flush=True)
    with torch.no_grad():
        chisq, _ = prob.forward_chisq(0)
    dof = 2 * vis.numel()
    if verbose:
        print('chi-square per real degree of freedom: %.3f (1 at the noise level); %d closure evaluations'
              % (2 * float(chisq) / dof, prob.closure_eval))
    return losses, 2 * float(chisq) / dof


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
