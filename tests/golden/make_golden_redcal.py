#!/usr/bin/env python3
"""
Golden vectors of redundant calibration (reference calibration.py: RedVisModel :877-1053, VisModel :1056-1209,
VisModelResponse :1212-1255, the degeneracy tools :2611-2915, BaseResponse.projection :181-212) on a 7-antenna hexagon
(autos + 21 cross baselines = 28, grouped by the reference's build_reds), 3 times, 5 channels, float64 / complex128.
TEST INFRASTRUCTURE ONLY, like make_golden.py, whose bootstrap it reuses; writes tests/golden/redcal.npz, arrays only.

Every model case of redcal_common.MODEL_CASES records the parameters, the input, the output, a random cotangent and the
gradient of Re sum(out * conj(cot)) with respect to the parameters.

Finding (reference): build_reds keys bl2red by antenna-pair tuples, RedVisModel.get_bl_idx looks baselines up by the numbers
of vd._blnums (:1010): the dictionary of build_reds cannot be used as it is.  The fixtures hand the reference a dictionary
keyed by baseline numbers; the restatement accepts either.
Finding (reference): the time index cache needs the response to know the time axis (:327-336), as for JonesModel.
Finding (reference): redcal_degen_vis decides which parameters are present by the truth value of the tensors (:2899-2904),
which only single-element tensors have, and evaluates bool(phs_slope) (two elements at least) whenever phs_slope is given: only
abs_amp alone, with one time and one channel, runs.  That call is recorded (dvis_amp1); the general result is recorded from
the reference's own redcal_degen_gains, as g_1 conj(g_2) exp(abs_amp) per baseline (dvis_both), which is what the function
states it computes.
Finding (reference): the weighted branch of compute_redcal_degen_vis names variables that do not exist (:2846); only the
unweighted call is recorded.

Usage:  python tests/golden/make_golden_redcal.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg    # noqa: E402
import redcal_common as rc  # noqa: E402


def gen_redcal(ba):
    cal = mg.load_calibration_module(ba)
    rng = np.random.default_rng(73)
    Nt, Nf = rc.NT, rc.NF
    freqs = torch.linspace(120e6, 180e6, Nf)
    times = torch.as_tensor(2459861.0 + np.arange(Nt) * 10.0 / 1440)
    arr = mg.hex_array(ba, 2, freqs)
    ants = arr.ants
    antpos = arr.to_antpos()
    bls = arr.get_bls(uniq_bls=False, keep_autos=True)
    Nbl = len(bls)
    assert Nbl == 28
    reds, _, bl2red = ba.telescope_model.build_reds(antpos, bls=bls, redtol=1.0)[:3]
    Nred = len(reds)
    blnums = ba.utils.ants2blnum(bls)
    bl2red_num = {int(n): bl2red[bl] for n, bl in zip(blnums, bls)}
    red = np.array([bl2red[bl] for bl in bls])

    def cx(*shape):
        return torch.as_tensor(rng.normal(size=shape) + 1j * rng.normal(size=shape))

    def fl(*shape):
        return torch.as_tensor(rng.normal(size=shape))

    def visdata(data, tsel=None, bsel=None):
        vd = ba.dataset.VisData()
        vd.setup_meta(None, antpos)
        b = bls if bsel is None else [bls[i] for i in bsel]
        t = times if tsel is None else times[tsel]
        if bsel is not None:
            data = data[:, :, bsel]
        if tsel is not None:
            data = data[:, :, :, tsel]
        vd.setup_data(b, t, freqs, pol='ee', data=data.clone())
        return vd

    out = dict(freqs=freqs, times=times, antvecs=arr.antvecs, ants=np.array(ants), bls=np.array(bls), red=red, Nred=np.array(Nred),
               vis=cx(1, 1, Nbl, Nt, Nf))
    for tag, (cls, ptype, kw) in rc.MODEL_CASES.items():
        rows = Nred if (cls == 'RedVisModel' and not kw.get('full')) else Nbl
        shape = (1, 1, rows, Nt, Nf, 2)
        p = 0.5 * fl(*shape)
        p0 = 0.3 * fl(*shape) if kw.get('p0') else None
        R = cal.VisModelResponse(param_type=ptype, times=times)
        if cls == 'RedVisModel':
            model = cal.RedVisModel(p.clone(), bl2red_num, R=R, p0=None if p0 is None else p0.clone())
        else:
            model = cal.VisModel(p.clone(), R=R, p0=None if p0 is None else p0.clone(), blnums=torch.as_tensor(blnums))
        vd = visdata(out['vis'], tsel=kw.get('tsel'), bsel=kw.get('bsel'))
        vout = model(vd, undo=bool(kw.get('undo')))
        cot = cx(*vout.data.shape)
        (vout.data * cot.conj()).real.sum().backward()
        out.update({'p_' + tag: p, 'vout_' + tag: vout.data.detach(), 'cot_' + tag: cot, 'g_' + tag: model.params.grad.clone()})
        if p0 is not None:
            out['p0_' + tag] = p0

    # degeneracies of gains: moderate amplitudes, phases well inside (-pi, pi) so that the phase fit sees no wrap
    gains = torch.exp(0.2 * fl(1, 1, len(ants), Nt, Nf) + 0.3j * fl(1, 1, len(ants), Nt, Nf))
    wg = torch.as_tensor(rng.uniform(0.5, 2.0, len(ants)))
    out.update(gains=gains, wgts_ant=wg)
    for tag, w in (('u', None), ('w', wg)):
        a, s = cal.compute_redcal_degen(gains, ants, antpos, wgts=w)
        out['degen_amp_' + tag], out['degen_phs_' + tag] = a, s
        out['degen_gains_' + tag] = cal.redcal_degen_gains(abs_amp=a, phs_slope=s, ants=ants, antpos=antpos)
        ng, nv, dg = cal.remove_redcal_degen(gains, ants, antpos, wgts=w)
        assert nv is None
        out['rm_gains_' + tag], out['rm_degen_' + tag] = ng, dg
    out['degen_gains_amp_only'] = cal.redcal_degen_gains(abs_amp=out['degen_amp_u'])
    cross = [i for i, bl in enumerate(bls) if bl[0] != bl[1]]
    out['cross'] = np.array(cross)
    redvis = cx(1, 1, len(cross), Nt, Nf)
    ng, nv, dg = cal.remove_redcal_degen(gains, ants, antpos, redvis=redvis, bls=[bls[i] for i in cross])
    new_degen = torch.exp(0.1 * fl(1, 1, len(ants), Nt, Nf) + 0.1j * fl(1, 1, len(ants), Nt, Nf))
    ng2, _, dg2 = cal.remove_redcal_degen(gains, ants, antpos, degen=new_degen)
    out.update(rm_redvis=redvis, rm_newvis=nv, rm_gains_rv=ng, new_degen=new_degen, rm_gains_nd=ng2, rm_degen_nd=dg2)

    # degeneracies of visibilities (cross baselines; tensor inputs)
    cbls = [bls[i] for i in cross]
    dvis = torch.exp(0.2 * fl(1, 1, len(cross), Nt, Nf) + 0.3j * fl(1, 1, len(cross), Nt, Nf))
    a, s = cal.compute_redcal_degen_vis(dvis, bls=cbls, antpos=antpos)
    out.update(dvis=dvis, dvis_amp=a, dvis_phs=s)
    a1 = torch.as_tensor(rng.normal(size=(1, 1, 1, 1, 1)) * 0.2 + 0.5)
    out['dvis_amp1_in'], out['dvis_amp1'] = a1, cal.redcal_degen_vis(abs_amp=a1)
    g = cal.redcal_degen_gains(abs_amp=None, phs_slope=s, ants=ants, antpos=antpos)
    i1, i2 = [ants.index(b[0]) for b in cbls], [ants.index(b[1]) for b in cbls]
    out['dvis_both'] = torch.exp(a) * g[:, :, i1] * g[:, :, i2].conj()

    # the degeneracy projection of a JonesResponse: output and gradient w.r.t. the (real-view) parameters
    pj = torch.view_as_real(gains.clone() * torch.exp(0.05 * cx(1, 1, len(ants), Nt, Nf))).clone()
    out['proj_p'] = pj.clone()
    for tag, kw in (('both', dict(abs_amp_gain=True, phs_slope_gain=True)), ('amp', dict(abs_amp_gain=True)),
                    ('phs_w', dict(phs_slope_gain=True, wgts_gain=wg)),
                    ('both_ref', dict(abs_amp_gain=True, phs_slope_gain=True, refant_idx=2))):
        R = cal.JonesResponse(param_type='com', antpos=antpos)
        R.setup_projection(**kw)
        pp = pj.clone().requires_grad_(True)
        y = R(pp)
        cot = cx(*y.shape)
        (y * cot.conj()).real.sum().backward()
        out.update({'proj_out_' + tag: y.detach(), 'proj_cot_' + tag: cot, 'proj_g_' + tag: pp.grad.clone()})
    mg.save('redcal', **out)


if __name__ == '__main__':
    torch.set_default_dtype(torch.float64)
    gen_redcal(mg.bootstrap_reference())
