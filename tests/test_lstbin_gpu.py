"""
GPU checks of the LST alignment stage (csrc/lstbin.hip through ops.vis_timeavg / rephase_phasor, telescope_model.vis_rephase,
VisData.lst_rephase / time_nn_interp / time_average) against the float64 restatement of lstbin_common and the reference's
recorded outputs (tests/golden/lstbin.npz).
"""
import numpy as np
import pytest
import torch

import lstbin_common as lc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CDT = {'f32': torch.complex64, 'f64': torch.complex128}
RDT = {'f32': torch.float32, 'f64': torch.float64}
_INPUTS = {}


def kernel_inputs(prec, Npp, Nf):
    """inputs of one shape, rounded to the working precision (the restatement sees what the kernel sees), made once"""
    key = (prec, Npp, Nf)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * Npp + Nf + (7 if prec == 'f64' else 0))
        shape = (Npp, lc.NBL, lc.NT, Nf)
        rd = np.float32 if prec == 'f32' else np.float64
        cd = np.complex64 if prec == 'f32' else np.complex128
        data = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(cd)
        wgts = rng.uniform(0.5, 2.0, size=shape).astype(rd)
        cov = rng.uniform(0.5, 2.0, size=shape).astype(rd)
        flags = rng.uniform(size=shape) < 0.5
        flags[:, 0, :3] = True
        freqs = np.linspace(120e6, 180e6, Nf) if Nf > 1 else np.array([150e6])
        tau_t = rng.uniform(-2e-7, 2e-7, size=(lc.NBL, lc.NT))                 # up to 36 turns
        gshape = lambda Nbin: (Npp, lc.NBL, Nbin, Nf)
        g = {Nbin: (rng.normal(size=gshape(Nbin)) + 1j * rng.normal(size=gshape(Nbin))).astype(cd) for Nbin in (3, 5)}
        _INPUTS[key] = dict(data=data, wgts=wgts, cov=cov, flags=flags, freqs=freqs, tau_t=tau_t, g=g,
                            tau_m=rng.uniform(-2e-7, 2e-7, size=(lc.NBL, 9)))
    return _INPUTS[key]


def to_dev(x):
    return None if x is None else torch.as_tensor(x).to(DEV)


def run(inp, bins, w, c, f, tau, by_member, g, data_t=None, wgts_t=None):
    from bayeslim_amd import ops
    data = (to_dev(inp['data']) if data_t is None else data_t).detach().requires_grad_(True)
    wg = (to_dev(inp['wgts']) if wgts_t is None else wgts_t) if w else None
    out = ops.vis_timeavg(data, ops.TimeAvgPlan(bins, lc.NT), wgts=wg, cov=to_dev(inp['cov']) if c else None,
                          flags=to_dev(inp['flags']) if f else None, tau=to_dev(tau), freqs=to_dev(inp['freqs']),
                          tau_by_member=by_member)
    gd, = torch.autograd.grad(out[0], data, to_dev(g))
    return (out[0].detach(),) + tuple(out[1:]), gd


@pytest.mark.parametrize('Npp', lc.NPP)
@pytest.mark.parametrize('prec,Nf', [(p, n) for p in ('f32', 'f64') for n in lc.NF[p]])
def test_forward_and_backward_against_the_restatement(prec, Nf, Npp):
    """every bin table x (weights, cov, flags, rephasing): forward at 1e-5 (float32) / 1e-12 (float64) of max|V|, backward
    at 1e-4 / 1e-10 of the maximum of the float64 adjoint, the adjoint identity in float64, equal bits on two runs"""
    inp = kernel_inputs(prec, Npp, Nf)
    vmax = np.abs(inp['data']).max()
    worst = [0.0, 0.0, 0.0]
    for tname, bins in lc.BIN_TABLES.items():
        Nmem = sum(len(b) for b in bins)
        for w, c, f, r in lc.OPTIONS:
            by_member = r and tname in ('singleton', 'repeated')
            tau = None if not r else (inp['tau_m'][:, :Nmem] if by_member else inp['tau_t'])
            g = inp['g'][len(bins)]
            (avg, sum_w, avg_cov, avg_flag), gd = run(inp, bins, w, c, f, tau, by_member, g)
            ravg, rsw, rcov, rflag = lc.timeavg(inp['data'], bins, inp['wgts'] if w else None, inp['cov'] if c else None,
                                                inp['flags'] if f else None, tau, inp['freqs'], by_member)
            case = (tname, w, c, f, r)
            assert avg.dtype == CDT[prec] and sum_w.dtype == RDT[prec] and tuple(avg.shape) == ravg.shape
            e = np.abs(avg.cpu().numpy() - ravg).max() / vmax
            worst[0] = max(worst[0], e)
            assert e <= lc.TOL_FWD[prec], (case, e)
            assert np.abs(sum_w.cpu().numpy() - rsw).max() <= lc.TOL_FWD[prec] * rsw.max(), case
            assert (avg_cov is None) == (not c) and (avg_flag is None) == (not f)
            if c:
                assert np.abs(avg_cov.cpu().numpy() - rcov).max() <= lc.TOL_FWD[prec] * rcov.max(), case
            if f:
                assert avg_flag.dtype == torch.bool and (avg_flag.cpu().numpy() == rflag).all(), case
            rgd = lc.timeavg_adjoint(g, bins, lc.NT, rsw, inp['wgts'] if w else None, tau, inp['freqs'], by_member)
            e = np.abs(gd.cpu().numpy() - rgd).max() / np.abs(rgd).max()
            worst[1] = max(worst[1], e)
            assert e <= lc.TOL_BWD[prec], (case, e)
            if tname == 'dropped':
                assert (gd[:, :, 4] == 0).all(), case                                    # a time in no bin: no gradient
            if prec == 'f64':
                lhs = np.vdot(avg.cpu().numpy(), g).real
                rhs = np.vdot(inp['data'], gd.cpu().numpy()).real
                worst[2] = max(worst[2], abs(lhs - rhs) / max(abs(lhs), 1.0))
                assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.abs(inp['data']).size ** 0.5), (case, lhs, rhs)
            (avg2, sum_w2, avg_cov2, avg_flag2), gd2 = run(inp, bins, w, c, f, tau, by_member, g)
            assert torch.equal(torch.view_as_real(avg), torch.view_as_real(avg2)) and torch.equal(sum_w, sum_w2), case
            assert torch.equal(torch.view_as_real(gd), torch.view_as_real(gd2)), case
            assert (not c or torch.equal(avg_cov, avg_cov2)) and (not f or torch.equal(avg_flag, avg_flag2)), case
    print('lstbin %s Npp %d Nf %d: fwd %.2e  bwd %.2e  adjoint %.2e' % (prec, Npp, Nf, *worst))


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_a_misaligned_base_gives_the_same_bits(prec):
    """Nf a multiple of the lane width: aligned tensors take 16-byte accesses; the same values at a base one (real) element
    off 16 bytes take element accesses -- forward and backward give equal bits"""
    Nf = lc.GROUP_F[prec]
    inp = kernel_inputs(prec, 4, Nf)

    def shifted(x):
        x = to_dev(x)
        real = torch.view_as_real(x) if x.is_complex() else x
        buf = torch.empty(real.numel() + 2, dtype=real.dtype, device=DEV)
        k = 1 if real.dtype == torch.float64 or not x.is_complex() else 2         # complex64: one element; float64: one real
        if x.is_complex() and real.dtype == torch.float64:
            return x, False                                                      # a complex128 view cannot start off 16 bytes
        v = buf[k:k + real.numel()].view(real.shape)
        v.copy_(real)
        return (torch.view_as_complex(v) if x.is_complex() else v), True

    d_al, w_al = to_dev(inp['data']), to_dev(inp['wgts'])
    d_off, moved_d = shifted(inp['data'])
    w_off, moved_w = shifted(inp['wgts'])
    assert d_al.data_ptr() % 16 == 0 and w_al.data_ptr() % 16 == 0
    assert w_off.data_ptr() % 16 != 0 and moved_w and (d_off.data_ptr() % 16 != 0) == moved_d
    for tname in ('full', 'repeated'):
        bins = lc.BIN_TABLES[tname]
        g = inp['g'][len(bins)]
        out_a, gd_a = run(inp, bins, True, True, True, inp['tau_t'], False, g, data_t=d_al, wgts_t=w_al)
        out_o, gd_o = run(inp, bins, True, True, True, inp['tau_t'], False, g, data_t=d_off, wgts_t=w_off)
        for a, o in zip(out_a, out_o):
            assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(o) if o.is_complex() else o), tname
        assert torch.equal(torch.view_as_real(gd_a), torch.view_as_real(gd_o)), tname


def fixture_tol(prec):
    return lc.TOL_FWD[prec] + lc.FACTOR * lc.RESTATEMENT


@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_vis_rephase_matches_the_fixture(prec):
    from bayeslim_amd import telescope_model as tm
    for name, (dlst, lat) in lc.REPHASE_CASES.items():
        rec = lc.recorded('rephase', name)['phasor']
        got = tm.vis_rephase(torch.as_tensor(dlst), lat, torch.as_tensor(lc.fix_blvecs()),
                             torch.as_tensor(lc.FIX_FREQS, dtype=RDT[prec], device=DEV))
        assert got.dtype == CDT[prec] and tuple(got.shape) == rec.shape, name
        assert np.abs(got.cpu().numpy() - rec).max() <= fixture_tol(prec), name


def make_vd(prec, pol, times, data, icov=None, cov=None, flags=None):
    from bayeslim_amd import dataset, telescope_model, utils
    vd = dataset.VisData()
    vd.setup_meta(telescope=telescope_model.TelescopeModel((lc.FIX_LON, lc.FIX_LAT)),
                  antpos=utils.AntposDict(lc.FIX_ANTS, torch.as_tensor(np.asarray(lc.FIX_ANTVECS))))
    R = lambda x: None if x is None else torch.as_tensor(x).to(RDT[prec]).to(DEV)
    vd.setup_data(lc.FIX_BLS, torch.as_tensor(times), torch.as_tensor(lc.FIX_FREQS, device=DEV), pol=pol,
                  data=torch.as_tensor(data).to(CDT[prec]).to(DEV), flags=to_dev(flags), cov=R(cov), cov_axis=None, icov=R(icov))
    return vd


def outputs(vd):
    out = {'data': vd.data.detach().cpu().numpy(), 'times': np.asarray(vd.times.cpu())}
    for k in ('flags', 'cov', 'icov'):
        if getattr(vd, k) is not None:
            out[k] = getattr(vd, k).cpu().numpy()
    return out


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('kind,name', lc.fixture_cases())
def test_visdata_methods_match_the_fixture(kind, name, prec, monkeypatch):
    """lst_rephase, time_nn_interp and time_average against the reference's records: data, flags, times, cov and icov"""
    from bayeslim_amd import telescope_model
    G = lc.golden()
    monkeypatch.setattr(telescope_model, 'JD2LST', lc.jd2lst)                   # the LST under which the records were made
    if kind == 'lstr':
        pol, dlst = lc.LSTR_CASES[name]
        vd = make_vd(prec, pol, lc.fix_times(lc.FIX_JD0), G['lstr_%s_data' % name])
        keep = vd.data
        out = vd.lst_rephase(dLST=torch.as_tensor(dlst), inplace=False)
        assert out is not vd and vd.data is keep
    elif kind == 'nn':
        pol, jd0, offs, rephase = lc.NN_CASES[name]
        vd = make_vd(prec, pol, G[name + '_times'], G[name + '_data'], G[name + '_icov'], G[name + '_cov'], G[name + '_flags'])
        out = vd.time_nn_interp(G[name + '_lsts'], rephase=rephase, inplace=True)
        assert out is vd and vd.Ntimes == len(offs)
    else:
        pol, time_inds, use_icov, use_cov, use_flags, rephase = lc.AVG_CASES[name]
        key = 'avg_' + name
        vd = make_vd(prec, pol, G[key + '_times'], G[key + '_data'], G.get(key + '_icov'), G.get(key + '_cov'), G.get(key + '_flags'))
        out = vd.time_average(time_inds=time_inds, rephase=rephase, inplace=True)
        assert out is vd and out.cov_axis is None
    tol = {'times': 1e-15}
    lc.compare(outputs(out), lc.recorded(kind, name), lambda k: tol.get(k, fixture_tol(prec)))


def test_time_average_falls_back_to_average_data_for_broadcast_weights():
    """weights that are not of the data's full shape go through average_data, as before: same numbers as the fused path fed
    with the expanded weights"""
    G = lc.golden()
    key = 'avg_bins_icov'
    w = torch.as_tensor(G[key + '_icov'][:, :, :, :, :1], device=DEV)
    tinds = lc.AVG_CASES['bins_icov'][1]
    a = make_vd('f64', None, G[key + '_times'], G[key + '_data'], flags=G[key + '_flags']).time_average(tinds, wgts=w, rephase=True)
    b = make_vd('f64', None, G[key + '_times'], G[key + '_data'], flags=G[key + '_flags']).time_average(
        tinds, wgts=w.expand(a.data.shape[:3] + (lc.FIX_NT, lc.FIX_NF)).contiguous(), rephase=True)
    assert lc.rel_err(a.data.cpu().numpy(), b.data.cpu().numpy()) <= 1e-12 and torch.equal(a.flags, b.flags)


def test_rime_point_source_rephased_to_the_first_integration():
    """the reference's own check (tests/test_dataset.py, test_vis_rephase): in a RIME simulation of one point source, every
    integration rephased to the first keeps its visibility phase within 1 rad of the first integration's, while the
    unrephased phase does not.  The reference's phasor cancels the fringe rotation to first order in dLST; the residual is
    second order, 2 sin(lat) cos(lat) (1 - cos dLST) b_N nu / c turns.  Geometry chosen so that this is below the bound: the
    source transits the zenith at the first integration, 10 integrations over 0.01 day (dLST <= 3.6 deg), a 19-antenna hexagon
    of 30 m spacing (b_N <= 104 m), 200 MHz at most: 0.12 turn = 0.76 rad (a float64 numpy model of the same gives 0.759);
    the unrephased phase runs through 27 rad"""
    from bayeslim_amd import sky_model, beam_model, rime_model, telescope_model, utils
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        freqs = torch.linspace(100e6, 200e6, 16, device=DEV)
        times = np.linspace(2458168.02, 2458168.03, 10)
        tel = telescope_model.TelescopeModel((lc.FIX_LON, lc.FIX_LAT))
        ants, vecs = utils._make_hex(3, D=30)
        arr = telescope_model.ArrayModel(utils.AntposDict(ants, vecs), freqs=freqs, device=DEV)
        ra, dec = np.array([float(telescope_model.JD2LST(times[0], lc.FIX_LON))]), np.array([lc.FIX_LAT])
        R = sky_model.PointSkyResponse(freqs, freq_mode='powerlaw', f0=freqs[0], device=DEV)
        sky = sky_model.PointSky(torch.tensor([1.0, -2.2], device=DEV).reshape(1, 1, 2, 1),           # amplitude, spectral index
                                 torch.as_tensor(np.stack([ra, dec]), device=DEV), R=R, parameter=False, name='ptsky')
        beam = beam_model.PixelBeam(torch.ones(1, 1, 1, 1, 1, device=DEV) * 14.0, freqs, R=beam_model.AiryResponse(powerbeam=True),
                                    pol='e', powerbeam=True, fov=180, parameter=False)
        bls = arr.get_bls(uniq_bls=True, keep_autos=False)
        rime = rime_model.RIME(sky, tel, beam, arr, bls, times, freqs)
        for t in times:
            tel.conv_cache[('ptsky', 1, float(t))] = torch.as_tensor(np.stack(telescope_model.eq2top(tel.location, t, ra, dec)))
        with torch.no_grad():
            vd = rime()
        out = vd.lst_rephase(dtime=torch.as_tensor(times[0] - times), inplace=False)
        drift = lambda d: (d / d[:, :, :, :1]).angle().abs().max().item()
        raw, reph = drift(vd.data), drift(out.data)
        print('phase drift: raw %.3f rad, rephased %.3f rad' % (raw, reph))
        assert reph < 1.0 and raw > 1.0
    finally:
        torch.set_default_dtype(old)
