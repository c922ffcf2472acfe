"""
GPU checks of the leapfrog kernel (csrc/hmc.hip) and of bayeslim_amd/sampler.py on it: rime_hmc_step against the restatement
of tests/hmc_common.py within its derived bounds, at the smallest shapes at which each mechanism can break (a lone element, a
ragged wave, one element either side of a work-group's span, three work-groups, and one element past the largest grid, where
the chunk loop and the second reduction stage both go round more than once), misaligned bases, the reproducibility of the
energy, then leapfrog, whole chains with their decisions and dual averaging against the reference's record, the order of
the integrator, and Potential over a LogProb.
"""
import numpy as np
import pytest
import torch

import hmc_common as hc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = (torch.float32, torch.float64)
# (kick, drift, energy) in units of the step: the three stages of a trajectory and the energy-only pass
STAGES = ((0.5, 1.0, False), (1.0, 1.0, False), (0.5, 0.0, True), (0.0, 0.0, True))
STEP = 0.37                                      # folded into the launch scalars: T(kick) is a rounding of its own in float32
TOL = max(hc.FACTOR * hc.LEAP_RESTATEMENT, hc.FLOOR)
TOL_CHAIN = max(hc.FACTOR * hc.CHAIN_RESTATEMENT, hc.FLOOR)


def span(dtype):
    from bayeslim_amd import sampler
    return sampler.STEP_SPAN[dtype]


def vec(rng, N, dtype, offset=0, positive=False):
    x = rng.uniform(0.5, 2.0, N) if positive else rng.normal(size=N)
    buf = torch.empty(N + offset, dtype=dtype, device=DEV)
    buf[offset:] = torch.as_tensor(x).to(dtype)
    return buf[offset:]


def launch(q, p, g, eps, c, kick, drift, energy):
    """one launch on copies; returns (q, p, E) as the kernel left them"""
    from bayeslim_amd import sampler
    q, p = q.clone(), p.clone()
    e = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV) if energy else None
    sampler.hmc_step(q if drift else None, p, g if kick else None, eps, c, kick, drift, e)
    return q, p, (float(e) if energy else None)


def check(q, p, g, eps, c, kick, drift, energy, dtype):
    """worst error / bound of one launch for p, q and the energy"""
    q1, p1, E1 = launch(q, p, g, eps, c, kick, drift, energy)
    qo, po, Eo = hc.oracle_step(q, p, g, eps, c, kick, drift, dtype)
    Bp = hc.p_bound(p, g, eps, kick, dtype)
    rp = hc.ratio(hc._ld(p1) - po, Bp)
    rq = hc.ratio(hc._ld(q1) - qo, hc.q_bound(q, po, Bp, eps, c, drift, dtype))
    rE = 0.0
    if energy:
        B = hc.energy_bound(po, Bp, c, dtype, float(Eo))
        rE = abs(E1 - float(Eo)) / B if B > 0 else (0.0 if E1 == float(Eo) else float('inf'))
    if not kick:
        assert torch.equal(p1, p)
    if not drift:
        assert torch.equal(q1, q)
    return rp, rq, rE


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_step_against_the_oracle(dtype):
    rng = np.random.default_rng(21)
    S = span(dtype)
    worst = np.zeros(3)
    for N in (1, 63, S - 1, S, S + 1, 2 * S + 5):
        q, p, g = vec(rng, N, dtype), vec(rng, N, dtype), vec(rng, N, dtype)
        for eps in (None, vec(rng, N, dtype, positive=True)):
            for c in (None, vec(rng, N, dtype, positive=True)):
                for kick, drift, energy in STAGES:
                    r = check(q, p, g, eps, c, kick * STEP, drift * STEP, energy, dtype)
                    worst = np.maximum(worst, r)
                    assert max(r) <= 1.0, (N, eps is not None, c is not None, kick, drift, energy, r)
    print('%s: worst error / bound  p %.3f  q %.3f  energy %.3f' % (dtype, *worst))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_step_beyond_the_largest_grid(dtype):
    """one element more than (most work-groups) x SPAN: a work-group takes a second chunk, a lane of the second reduction
    stage adds 16 partials; the last element is the lone element of the last chunk"""
    from bayeslim_amd import sampler
    rng = np.random.default_rng(22)
    N = sampler.STEP_MAXBLOCKS * span(dtype) + 1
    q, p, g = vec(rng, N, dtype), vec(rng, N, dtype), vec(rng, N, dtype)
    eps, c = vec(rng, N, dtype, positive=True), vec(rng, N, dtype, positive=True)
    for kick, drift, energy in ((1.0, 1.0, False), (0.5, 0.0, True)):
        r = check(q, p, g, eps, c, kick * STEP, drift * STEP, energy, dtype)
        print('%s N = %d (%.1f, %.1f, %s): error / bound  p %.3f  q %.3f  energy %.3f' % (dtype, N, kick, drift, energy, *r))
        assert max(r) <= 1.0
    _, p1, _ = launch(q, p, g, eps, c, STEP, STEP, False)
    assert float(p1[-1]) != float(p[-1])                                  # the tail element was reached


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_misaligned_bases_give_the_same_bits(dtype):
    rng = np.random.default_rng(23)
    for N in (63, span(dtype) + 1, 2 * span(dtype) + 5):
        al = [vec(rng, N, dtype), vec(rng, N, dtype), vec(rng, N, dtype), vec(rng, N, dtype, positive=True),
              vec(rng, N, dtype, positive=True)]

        def shifted(t):
            buf = torch.empty(N + 1, dtype=dtype, device=DEV)
            buf[1:] = t
            return buf[1:]
        mis = [shifted(t) for t in al]
        assert all(t.data_ptr() % 16 == 0 for t in al) and all(t.data_ptr() % 16 != 0 for t in mis)
        for kick, drift, energy in STAGES + ((1.0, 1.0, True),):
            want = launch(*al, kick * STEP, drift * STEP, energy)
            # launch() clones: the clones of misaligned views are aligned, so shift the clones instead
            from bayeslim_amd import sampler
            q, p = shifted(mis[0]), shifted(mis[1])
            e = torch.zeros(1, dtype=torch.float64, device=DEV) if energy else None
            sampler.hmc_step(q if drift else None, p, mis[2] if kick else None, mis[3], mis[4], kick * STEP, drift * STEP, e)
            assert q.data_ptr() % 16 != 0 and p.data_ptr() % 16 != 0
            assert torch.equal(q, want[0]) and torch.equal(p, want[1]) and (not energy or float(e) == want[2])
            # a mixture: only the momentum and the step size misaligned
            q2, p2 = al[0].clone(), shifted(al[1])
            e2 = torch.zeros(1, dtype=torch.float64, device=DEV) if energy else None
            sampler.hmc_step(q2 if drift else None, p2, al[2] if kick else None, mis[3], al[4], kick * STEP, drift * STEP, e2)
            assert torch.equal(q2, want[0]) and torch.equal(p2, want[1]) and (not energy or float(e2) == want[2])


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_energy_is_reproducible_and_the_same_fused_or_alone(dtype):
    from bayeslim_amd import sampler
    rng = np.random.default_rng(24)
    for N in (2 * span(dtype) + 5, sampler.STEP_MAXBLOCKS * span(dtype) + 1):
        p, g, c = vec(rng, N, dtype), vec(rng, N, dtype), vec(rng, N, dtype, positive=True)
        fused = [launch(p, p, g, None, c, 0.5 * STEP, 0.0, True) for _ in range(3)]
        assert len({f[2] for f in fused}) == 1 and all(torch.equal(f[1], fused[0][1]) for f in fused)
        alone = [launch(p, fused[0][1], None, None, c, 0.0, 0.0, True)[2] for _ in range(3)]
        assert set(alone) == {fused[0][2]}
        assert fused[0][2] > 0 and np.isfinite(fused[0][2])


# ----------------------------------------------------------------------------------------------------- against the record
def to_dev(d):
    return {k: torch.tensor(v, device=DEV) for k, v in d.items()}          # copies: the fixtures are never modified


def rel(got, ref):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize('name', list(hc.LEAP_CASES))
def test_leapfrog_against_the_reference(name, monkeypatch):
    """float64 (complex128 for the complex key, through its real view) on the GPU against the recorded outputs and states;
    N steps are N + 1 launches"""
    from bayeslim_amd import sampler
    from bayeslim_amd.paramdict import ParamDict
    g = hc.golden()
    cont, keys, q0, p0, a, eps, cov = hc.leap_inputs(g, name)
    at = to_dev(a)
    launches = []
    real_step = sampler.hmc_step
    monkeypatch.setattr(sampler, 'hmc_step', lambda *args, **kw: (launches.append(args[5:7]), real_step(*args, **kw))[1])

    def dUdq(q, Ucache=None):
        if isinstance(q, torch.Tensor):
            U, gr = hc.grad_U(at[keys[0]], q)
        else:
            U, gr = 0, {}
            for k in q:
                Uk, gr[k] = hc.grad_U(at[k], q[k])
                U = U + Uk
            gr = ParamDict(gr)
        if Ucache is not None:
            Ucache.append(U)
        return gr

    states = [] if name == hc.LEAP_STATES else None
    if cont == 'tensor':
        k = keys[0]
        q, p = to_dev(q0)[k], to_dev(p0)[k]
        e = eps if isinstance(eps, float) else to_dev(eps)[k]
        out = sampler.leapfrog(q, p, dUdq, e, hc.LEAP_N, cov_L=None if cov is None else to_dev(cov)[k])
        assert out[0] is q and out[1] is p
        q, p = {k: q}, {k: p}
    else:
        q, p = ParamDict(to_dev(q0)), ParamDict(to_dev(p0))
        held = q[keys[0]]
        e = eps if isinstance(eps, float) else ParamDict(to_dev(eps))
        sampler.leapfrog(q, p, dUdq, e, hc.LEAP_N, cov_L=None if cov is None else ParamDict(to_dev(cov)), states=states)
        assert q[keys[0]] is held                                         # in place
    assert len(launches) == hc.LEAP_N + 1
    s = hc.EPS_SCALAR if isinstance(eps, float) else 1.0
    assert launches == [(0.5 * s, s)] + [(s, s)] * (hc.LEAP_N - 1) + [(0.5 * s, 0.0)]
    worst = 0.0
    for k in keys:
        worst = max(worst, rel(q[k], g['leap_%s_q_%s' % (name, k)]), rel(p[k], g['leap_%s_p_%s' % (name, k)]))
        assert q[k].dtype == (torch.complex128 if k == 'w' else torch.float64)
        if states is not None:
            assert len(states) == hc.LEAP_N + 1
            worst = max(worst, rel(torch.stack([st[0][k] for st in states]), g['leap_%s_states_q_%s' % (name, k)]),
                        rel(torch.stack([st[1][k] for st in states]), g['leap_%s_states_p_%s' % (name, k)]))
    if states is not None:
        U = np.array([np.nan if st[2] is None else float(st[2]) for st in states])
        ref = g['leap_%s_states_U' % name]
        assert not np.isnan(ref).any() and rel(U, ref) <= TOL
    print('leapfrog %s on the GPU: %.3e' % (name, worst))
    assert worst <= TOL


def gpu_hmc(g, dHmax, eps0=None):
    from bayeslim_amd import sampler
    from bayeslim_amd.paramdict import ParamDict
    a, x0, cov, hess, draws = [to_dev(d) for d in hc.chain_inputs(g)]

    def potential(x):
        U, gr = 0, {}
        for k in x:
            Uk, gr[k] = hc.grad_U(a[k], x[k])
            U = U + Uk
        return U, ParamDict(gr)

    count = {k: 0 for k in x0}

    def dist(k):
        def draw():
            count[k] += 1
            return draws[k][count[k] - 1].clone()
        return draw

    eps = ParamDict({k: torch.tensor(v, dtype=torch.float64, device=DEV) for k, v in (eps0 or hc.CHAIN['eps']).items()})
    return sampler.HMC(potential, ParamDict(x0), eps, cov_L=ParamDict(cov), hess_L=ParamDict(hess), Nstep=hc.CHAIN['Nstep'],
                       pdist={k: dist(k) for k in x0}, dHmax=dHmax)


@pytest.mark.parametrize('tag', ['b', 'c'])
def test_chain_against_the_reference(tag):
    """sampler.HMC in float64 on the GPU on the recorded chains: identical accept and divergence decisions, the floating-point
    record within FACTOR x the recorded discrepancy of the restatement (floor hc.FLOOR)"""
    g = hc.golden()
    np.random.seed(hc.CHAIN['seed'])
    s = gpu_hmc(g, hc.CHAIN['dHmax_' + tag])
    recs = []
    for i in range(hc.CHAIN['steps']):
        evals = s.fn_evals
        accept, prob = s.step()
        assert s.fn_evals == evals + hc.CHAIN['Nstep'] + 1
        s._acceptances.append(bool(accept))
        s.append_chain(s.x, U=s._U)
        dH = s._last['H_end'] - s._last['H_start']
        recs.append(dict(accept=bool(accept), prob=float(prob), U=float(s._U), div=dH > s.dHmax, K_start=s._last['K_start'],
                         H_end=s._last['H_end'], x={k: s.x[k].cpu().numpy() for k in s.x},
                         p={k: s._traj.pv[k].cpu().numpy().copy() for k in s.x}))
    e = hc.chain_discrepancy(recs, g, tag)
    print('chain %s on the GPU: %.3e' % (tag, e))
    assert e <= TOL_CHAIN
    assert len(s.Uchain) == hc.CHAIN['steps'] and s.get_chain('u')['u'].shape == (hc.CHAIN['steps'],) + hc.SHAPES['u']


def test_dual_averaging_against_the_reference():
    """eps after Nadapt adapting moves against record 'd'.  The tolerance follows from the chains': log eps_i = mu - h_i sqrt(i) /
    gamma with h_i a convex combination of (target - prob_j), so |d log eps| <= sqrt(Nadapt) / gamma max|d prob|, and
    |d prob| = prob |d(H_start - H_end)| <= 2 TOL_CHAIN max|H|, each Hamiltonian being held to TOL_CHAIN relative to the
    largest recorded one (the same potential and start as chain 'b').  A slip in the recursion changes eps by tens of per cent."""
    g = hc.golden()
    tol = np.sqrt(hc.CHAIN['Nadapt']) / 0.05 * 2 * TOL_CHAIN * float(np.abs(g['chain_b_H_end']).max())
    np.random.seed(hc.CHAIN['seed'])
    s = gpu_hmc(g, hc.CHAIN['dHmax_b'], eps0=hc.dual_eps0())
    s.dual_averaging(hc.CHAIN['Nadapt'])
    worst = max(abs(float(s.eps[k]) - float(g['dual_eps_' + k])) / float(g['dual_eps_' + k]) for k in hc.CHAIN['keys'])
    print('dual averaging on the GPU: %.3e (tolerance %.3e)' % (worst, tol))
    assert worst <= tol < 1e-6


def test_leapfrog_is_second_order():
    """on the quadratic part alone: halving eps at a fixed trajectory length cuts |dH| by more than 2 (asymptotically 4)"""
    from bayeslim_amd import sampler
    g = hc.golden()
    a = torch.as_tensor(g['chain_a_v']).to(DEV)
    q0, p0 = torch.as_tensor(g['chain_x0_v']).to(DEV), torch.as_tensor(g['chain_draws_v'][0]).to(DEV)
    H = lambda q, p: float((a * q * q).sum() / 2 + (p * p).sum() / 2)
    dUdq = lambda q, Ucache=None: a * q
    dH = []
    for eps, N in ((0.1, 8), (0.05, 16), (0.025, 32)):
        q, p = q0.clone(), p0.clone()
        sampler.leapfrog(q, p, dUdq, eps, N)
        dH.append(abs(H(q, p) - H(q0, p0)))
    print('|dH| at eps = 0.1, 0.05, 0.025: %.3e %.3e %.3e' % tuple(dH))
    assert dH[0] > 2 * dH[1] > 4 * dH[2] > 0


def test_potential_over_a_logprob_and_two_moves():
    """Potential on the smallest RIME fixture (7 antennas, 10 point sources): U and the gradients are prob.closure()'s; an
    accepted move leaves the model at the new position, a refused one puts it back"""
    from bayeslim_amd import sky_model, beam_model, rime_model, optim, dataset, utils, telescope_model, sampler
    from bayeslim_amd.paramdict import ParamDict
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        g = load_golden('rime_c1')
        T = lambda x, dt=torch.float64: torch.as_tensor(np.asarray(x)).to(dt).to(DEV)
        freqs = T(g['freqs'])
        antpos = utils.AntposDict(g['ants'].tolist(), torch.as_tensor(g['antvecs'], dtype=torch.float64))
        arr = telescope_model.ArrayModel(antpos, freqs=freqs, cache_s=True, redtol=1.0, device=DEV)
        tel = telescope_model.TelescopeModel((21.42827, -30.72148))
        R = sky_model.PointSkyResponse(freqs, freq_mode='powerlaw', f0=freqs[0], device=DEV)
        sky = sky_model.PointSky(T(g['sky_params']) * 1.05, T(np.stack([g['ra'], g['dec']])), R=R, parameter=True, name='ptsky')
        beam = beam_model.PixelBeam(torch.ones(1, 1, 1, 1, 1, device=DEV) * float(g['airy_D']), freqs,
                                    R=beam_model.AiryResponse(powerbeam=True), pol='e', powerbeam=True, fov=180, parameter=False)
        sim_bls = [tuple(b) for b in g['sim_bls']]
        rime = rime_model.RIME(sky, tel, beam, arr, sim_bls, g['times'], freqs)
        Npix = g['zenaz'].shape[-1]
        for t, za in zip(g['times'], g['zenaz']):
            tel.conv_cache[('ptsky', Npix, float(t))] = torch.as_tensor(za, dtype=torch.float64)
        target = dataset.VisData()
        target.setup_data(sim_bls, torch.as_tensor(g['times']), freqs, pol='ee', data=T(g['vis'], torch.complex128),
                          icov=torch.ones(g['vis'].shape, device=DEV))
        prob = optim.LogProb(utils.Sequential(dict(rime=rime)), dataset.Dataset([target]), device=DEV)
        names = prob.named_params
        assert len(names) == 1
        name = names[0]
        pot = sampler.Potential(prob)
        close = lambda x, y: abs(float(x) - float(y)) <= 1e-12 * abs(float(y))      # two evaluations of the same point
        U, grad = pot()
        assert grad.keys() == names and float(U) > 0
        assert torch.equal(grad[name], prob[name].grad) and grad[name] is not prob[name].grad
        assert close(U, prob.closure()) and rel(grad[name], prob[name].grad.cpu().numpy()) <= 1e-12
        x0 = ParamDict({name: prob[name].detach().clone()})
        U2, grad2 = pot(x0 * 1.01)
        assert float(U2) != float(U) and torch.equal(prob[name].detach(), x0[name] * 1.01)
        assert torch.equal(grad2[name], prob[name].grad) and close(U2, prob.closure())

        scale = float(x0[name].abs().mean())
        np.random.seed(3)
        torch.manual_seed(3)
        s = sampler.HMC(pot, x0, 1e-6 * scale, Nstep=3)
        assert close(s._U, U)
        accept, p_acc = s.step()
        assert bool(accept) and float(p_acc) > 0.99
        assert not torch.equal(s.x[name], x0[name]) and torch.equal(prob[name].detach(), s.x[name])
        assert close(s._U, prob.closure())
        x1 = s.x[name].clone()
        s.eps = 1e3 * scale                                               # a step far too long: the move is refused
        accept, p_rej = s.step()
        assert not bool(accept) and not float(p_rej) > 1e-3
        assert torch.equal(s.x[name], x1) and torch.equal(prob[name].detach(), x1)
        assert s.fn_evals == 2 * (3 + 1) and isinstance(prob[name], torch.nn.Parameter)
    finally:
        torch.set_default_dtype(old)
