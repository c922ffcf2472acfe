"""
GPU checks of the tree-leaf kernels (csrc/nuts.hip) and of bayeslim_amd/nuts.py on them.  Kernels: rime_nuts_leaf_open and
rime_nuts_leaf_close bit for bit against the composition they replace (copies of the edge state and two launches of
rime_hmc_step), the two projections against the long-double restatement of tests/nuts_common.py within its derived bounds, at
the smallest shapes at which each mechanism can break (a lone element, a ragged wave, one element either side of a work-group's
span, three work-groups and a tail, and more chunks than work-groups, where the chunk loop and the second reduction stage both
go round more than once), misaligned bases, the untouched inputs, the sentinel without a far edge, reproducibility.  Sampler:
the three recorded chains of the reference with equal decisions, launch and evaluation counts, the criterion on a complex key,
tracked states, chain files, a Potential-backed move, and the float32 leaves within their bounds.
"""
import numpy as np
import pytest
import torch

import hmc_common as hc
import nuts_common as nc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = (torch.float32, torch.float64)
STEP = 0.37                                      # T(h) and T(h / 2) are roundings of their own in float32
TOL = nc.FACTOR * nc.NUTS_RESTATEMENT + nc.FLOOR
SENTINEL = -7.25


def span(dtype):
    from bayeslim_amd import sampler
    return sampler.STEP_SPAN[dtype]


def vec(rng, N, dtype, offset=0, positive=False):
    x = rng.uniform(0.5, 2.0, N) if positive else rng.normal(size=N)
    buf = torch.empty(N + offset, dtype=dtype, device=DEV)
    buf[offset:] = torch.as_tensor(x).to(dtype)
    return buf[offset:]


def leaf(q0, p0, g0, g1, eps, c, h, q_far, p_far, dtype, offset=0):
    """
    One leaf through the two kernels, checked against the composition from rime_hmc_step (bit for bit) and against the
    restatement (the projections, within their bounds); returns (q1, p1, out) as the kernels left them and the worst
    error / bound of the two projections.
    """
    from bayeslim_amd import nuts, sampler
    N = p0.numel()
    ins = [t for t in (q0, p0, g0, g1, eps, c, q_far, p_far) if t is not None]
    kept = [t.clone() for t in ins]
    new = lambda: torch.full((N + offset,), float('nan'), dtype=dtype, device=DEV)[offset:]
    q1, p1 = new(), new()
    nuts.leaf_open(q0, p0, g0, q1, p1, eps, c, h)
    qc, pc = q0.clone(), p0.clone()
    sampler.hmc_step(qc, pc, g0, eps, c, h / 2, h)
    assert torch.equal(q1, qc) and torch.equal(p1, pc)
    e = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV)
    pc2 = pc.clone()
    sampler.hmc_step(None, pc2, g1, eps, c, h / 2, 0.0, e)
    out = torch.full((3,), SENTINEL, dtype=torch.float64, device=DEV)
    nuts.leaf_close(q1, p1, g1, eps, c, h, q_far, p_far, out)
    assert torch.equal(q1, qc) and torch.equal(p1, pc2)
    out = out.tolist()
    assert out[0] == float(e) and np.isfinite(out[0])                      # the bits of rime_hmc_step's energy
    assert all(torch.equal(a, b) for a, b in zip(ins, kept))                # every input is as it was
    if q_far is None:
        assert out[1] == SENTINEL and out[2] == SENTINEL
        return q1, p1, out, (0.0, 0.0)
    po, (_, far, near) = nc.oracle_close(q1, pc, g1, eps, c, h, q_far, p_far, dtype)
    Bp = hc.p_bound(pc, g1, eps, h / 2, dtype)
    B = nc.dots_bound(q1, q_far, p_far, po, Bp, dtype)
    assert nc.within(out[1], far, B[0]) and nc.within(out[2], near, B[1]), (N, out, float(far), float(near), B)
    r = [abs(float(np.longdouble(o) - w)) / b if b > 0 else 0.0 for o, w, b in zip(out[1:], (far, near), B)]
    return q1, p1, out, tuple(r)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_leaf_against_the_composition_and_the_oracle(dtype):
    rng = np.random.default_rng(31)
    S = span(dtype)
    worst = np.zeros(2)
    for N in (1, 63, S - 1, S, S + 1, 3 * S + 17):
        q0, p0, g0, g1, qf, pf = [vec(rng, N, dtype) for _ in range(6)]
        for eps in (None, vec(rng, N, dtype, positive=True)):
            for c in (None, vec(rng, N, dtype, positive=True)):
                for h in (STEP, -STEP):
                    worst = np.maximum(worst, leaf(q0, p0, g0, g1, eps, c, h, qf, pf, dtype)[3])
        leaf(q0, p0, g0, g1, None, None, -STEP, None, None, dtype)           # no far edge: the sentinel stays
        q1, p1, out, _ = leaf(q0, p0, g0, g1, None, None, STEP, qf, pf, dtype)
        _, _, zero, _ = leaf(q0, p0, g0, g1, None, None, STEP, q1, pf, dtype)    # the far edge at the leaf itself: a span of zero
        assert zero[1] == 0.0 and zero[2] == 0.0
    print('%s: worst error / bound of the projections  far %.3f  near %.3f' % (dtype, *worst))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_leaf_with_more_chunks_than_work_groups(dtype):
    """1025 spans and five elements: a work-group takes a second chunk, a lane of the second stage adds 16 partials of each sum,
    the last five elements are alone in the last chunk; run twice: the same bits"""
    from bayeslim_amd import sampler
    rng = np.random.default_rng(32)
    N = (sampler.STEP_MAXBLOCKS + 1) * span(dtype) + 5
    q0, p0, g0, g1, qf, pf = [vec(rng, N, dtype) for _ in range(6)]
    eps, c = vec(rng, N, dtype, positive=True), vec(rng, N, dtype, positive=True)
    q1, p1, out, r = leaf(q0, p0, g0, g1, eps, c, -STEP, qf, pf, dtype)
    print('%s N = %d: error / bound of the projections  far %.3f  near %.3f' % (dtype, N, *r))
    q2, p2, out2, _ = leaf(q0, p0, g0, g1, eps, c, -STEP, qf, pf, dtype)
    assert torch.equal(q1, q2) and torch.equal(p1, p2) and out == out2
    assert float(p1[-1]) != float(p0[-1]) and float(q1[-1]) != float(q0[-1])  # the tail element was reached


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_misaligned_bases_give_the_same_bits(dtype):
    rng = np.random.default_rng(33)
    for N in (63, span(dtype) + 1, 3 * span(dtype) + 17):
        al = [vec(rng, N, dtype) for _ in range(4)] + [vec(rng, N, dtype, positive=True) for _ in range(2)] + [vec(rng, N, dtype) for _ in range(2)]

        def shifted(t):
            buf = torch.empty(N + 1, dtype=dtype, device=DEV)
            buf[1:] = t
            return buf[1:]
        mis = [shifted(t) for t in al]
        assert all(t.data_ptr() % 16 == 0 for t in al) and all(t.data_ptr() % 16 != 0 for t in mis)
        q0, p0, g0, g1, eps, c, qf, pf = al
        want = leaf(q0, p0, g0, g1, eps, c, STEP, qf, pf, dtype)
        for args, offset in ((mis, 1), (mis, 0), ([al[0], mis[1], al[2], mis[3], mis[4], al[5], mis[6], al[7]], 1)):
            q0, p0, g0, g1, eps, c, qf, pf = args
            got = leaf(q0, p0, g0, g1, eps, c, STEP, qf, pf, dtype, offset=offset)
            assert (got[0].data_ptr() % 16 != 0) == bool(offset)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2]


# ----------------------------------------------------------------------------------------------------- against the record
def to_dev(d, dtype=torch.float64):
    return {k: torch.tensor(v, device=DEV).to(dtype) for k, v in d.items()}      # copies: the fixtures are never modified


def gpu_nuts(g, tag, dtype=torch.float64, **kw):
    from bayeslim_amd import nuts
    from bayeslim_amd.paramdict import ParamDict
    a, x0, cov, hess, draws = [to_dev(d, dtype) for d in nc.chain_inputs(g)]
    cfg = dict(nc.CHAINS[tag], **kw)

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

    return nuts.NUTS(potential, ParamDict(x0), cfg['eps'], cov_L=ParamDict(cov), hess_L=ParamDict(hess), pdist={k: dist(k) for k in x0},
                     dHmax=cfg['dHmax'], max_tree_depth=cfg['max_tree_depth'], biased=cfg['biased'], track_states=cfg['track_states'],
                     sample_direction=cfg['sample_direction'])


def run_chain(s, monkeypatch, steps=nc.STEPS):
    """the moves of a chain as the records nuts_common.chain_discrepancy takes, with the launch count of every move"""
    log = dict(level=0)
    build, leaf_, rand = s._build, s._leaf, np.random.rand

    def _build(edge, direction, depth, H_start, far):
        if log['level'] == 0:
            log['rec']['dirs'].append(direction)
        log['level'] += 1
        try:
            return build(edge, direction, depth, H_start, far)
        finally:
            log['level'] -= 1

    def _leaf(edge, direction, H_start, far):
        t = leaf_(edge, direction, H_start, far)
        r = log['rec']
        r['leaf_K'].append(float(s._out[0]) + s._logdetM), r['leaf_H'].append(t.q_prop_H)
        r['leaf_minus'].append(t.left.minus_angle), r['leaf_plus'].append(t.left.plus_angle)
        return t

    def recording_rand():
        log['rec']['u'].append(rand())
        return log['rec']['u'][-1]

    monkeypatch.setattr(s, '_build', _build)
    monkeypatch.setattr(s, '_leaf', _leaf)
    monkeypatch.setattr(np.random, 'rand', recording_rand)
    recs = []
    for _ in range(steps):
        log['rec'] = rec = dict(u=[], dirs=[], leaf_K=[], leaf_H=[], leaf_minus=[], leaf_plus=[])
        evals, launches = s.fn_evals, s.launches
        s._base_tree = None
        accept, prob = s.step()
        restart = s._base_tree is None
        s._acceptances.append(bool(accept))
        s.append_chain(s.x, U=s._U)
        rec.update(accept=bool(accept), prob=float(prob), U=float(s._U), restart=restart, depth=s._last['tree_depth'],
                   H=float('nan') if restart else s._base_tree.q_prop_H, fn_evals=s.fn_evals - evals, launches=s.launches - launches,
                   x={k: s.x[k].cpu().numpy() for k in s.x}, nstates=0 if restart or s._base_tree.states is None else len(s._base_tree.states))
        recs.append(rec)
    monkeypatch.undo()
    return recs


@pytest.mark.parametrize('tag', list(nc.CHAINS))
def test_chain_against_the_reference(tag, monkeypatch, tmp_path):
    """nuts.NUTS in float64 on the GPU on the recorded chains: the reference's decisions (accept, restart, tree depth, fn_evals,
    directions, leaves, every uniform draw in its place), the floating-point record within FACTOR x the recorded discrepancy of
    the restatement plus FLOOR, two launches per leaf and one energy-only pass per move"""
    from bayeslim_amd import nuts
    g = nc.golden()
    np.random.seed(nc.CHAINS[tag]['seed'])
    s = gpu_nuts(g, tag)
    recs = run_chain(s, monkeypatch)
    e = nc.chain_discrepancy(recs, g, tag)
    print('chain %s on the GPU: %.3e (tolerance %.3e)' % (tag, e, TOL))
    assert e <= TOL
    assert [r['launches'] for r in recs] == [2 * len(r['leaf_K']) + 1 for r in recs]
    assert [r['fn_evals'] for r in recs] == [len(r['leaf_K']) + 1 for r in recs]
    assert [float(r['nstates']) for r in recs] == g['chain_%s_nstates' % tag].tolist()
    assert len(s.Uchain) == nc.STEPS and s.get_chain('u')['u'].shape == (nc.STEPS,) + hc.SHAPES['u']
    if tag == 'b':                                                   # tracked states: views of the shared leaf states, left to right
        t = s._base_tree
        assert t.states[0][0] is t.q_left and t.states[-1][0] is t.q_right and any(st[0] is t.q_prop for st in t.states)
        assert isinstance(t, nuts.TreeInfo) and s.is_turning(t) in (True, False)
    if tag == 'c':                                                   # the chain file and what a sampler reads back from it
        f = str(tmp_path / 'nuts_chain.npz')
        s.write_chain(f)
        t = gpu_nuts(g, tag)
        t.load_chain(f)
        assert [float(u) for u in t.Uchain] == [float(u) for u in s.Uchain] and t.fn_evals == s.fn_evals and len(t._acceptances) == nc.STEPS
        assert all(np.array_equal(np.asarray(t.chain[k]), np.asarray(s.chain[k])) for k in nc.KEYS)
        assert all(torch.equal(t.x[k], s.x[k].cpu()) for k in nc.KEYS)


def test_seeded_chain_is_reproducible_bit_for_bit(monkeypatch):
    g = nc.golden()
    runs = []
    for _ in range(2):
        np.random.seed(nc.CHAINS['a']['seed'])
        runs.append(run_chain(gpu_nuts(g, 'a'), monkeypatch, steps=3))
    for r0, r1 in zip(*runs):
        assert all(r0[n] == r1[n] for n in ('accept', 'prob', 'U', 'H', 'u', 'dirs', 'leaf_K', 'leaf_minus', 'leaf_plus'))
        assert all(np.array_equal(r0['x'][k], r1['x'][k]) for k in nc.KEYS)


def test_inherited_drivers_run():
    """sample and dual_averaging of sampler.HMC on the NUTS move"""
    g = nc.golden()
    np.random.seed(5)
    s = gpu_nuts(g, 'a', max_tree_depth=2, eps=0.03)            # dual averaging starts near ten times the step it is given
    s.sample(2)
    assert len(s.Uchain) == 2 and 0.0 <= float(s.accept_ratio) <= 1.0
    eps = float(s.eps)
    s.dual_averaging(2)
    assert np.isfinite(float(s.eps)) and float(s.eps) != eps and s.fn_evals == 4 * (1 + 3)


def test_uturn_on_a_complex_key_through_the_kernel():
    """states on a real and a complex key (the complex one behind a gap of the flat layout) where the reference's criterion is
    true and where it is false: the kernel's two projections have the signs of hoffman_uturn's for either direction"""
    from bayeslim_amd import nuts, sampler
    from bayeslim_amd.paramdict import ParamDict
    rng = np.random.default_rng(35)
    cplx = lambda n: torch.tensor(rng.normal(size=n) + 1j * rng.normal(size=n), device=DEV)
    real = lambda n: torch.tensor(rng.normal(size=n), device=DEV)
    state = lambda: ParamDict({'v': real(3), 'w': cplx(17)})
    lay = sampler._Layout(state())
    assert lay.cplx['w'] and lay.slices['w'].start == 4 and lay.N == 4 + 34
    flat = lambda x: lay.pack(x, lay.new())
    q_far, q1 = state(), state()
    along = q1 - q_far
    zero = flat(along * 0)
    seen = set()
    for p_far, p1 in ((along, along), (along * -1.0, along), (along, along * -1.0), (state(), state()), (state(), state())):
        out = torch.zeros(3, dtype=torch.float64, device=DEV)
        buf = flat(p1)
        nuts.leaf_close(flat(q1), buf, zero, None, None, 1.0, flat(q_far), flat(p_far), out)    # a zero gradient: p1 stays
        assert torch.equal(buf, flat(p1))
        K, far, near = out.tolist()
        forward = sampler.hoffman_uturn(q_far, q1, p_far, p1)                   # direction +1: the far edge is q_minus
        backward = sampler.hoffman_uturn(q1, q_far, p1, p_far)                  # direction -1: the far edge is q_plus
        assert ((far < 0) or (near < 0)) == forward and ((-near < 0) or (-far < 0)) == backward
        ref = sum(float(((q1[k] - q_far[k]).conj().ravel() @ p_far[k].ravel()).real) for k in q1)
        assert abs(far - ref) <= 1e-13 * float(sum((q1[k] - q_far[k]).abs().ravel() @ p_far[k].abs().ravel() for k in q1))
        assert abs(K - float(sum((p1[k].abs() ** 2).sum() for k in p1)) / 2) <= 1e-13 * K
        seen.add(forward)
    assert seen == {True, False}


def test_float32_leaves_within_their_bounds(monkeypatch):
    """the first move of chain 'a' in float32: every launch of the move against the restatement on the operands it was given
    (p and q of open, p, the energy and the projections of close); no decision is compared"""
    from bayeslim_amd import nuts
    g = nc.golden()
    dt = torch.float32
    np.random.seed(nc.CHAINS['a']['seed'])
    s = gpu_nuts(g, 'a', dtype=dt)
    opened, closed, worst = nuts.leaf_open, nuts.leaf_close, np.zeros(5)

    def leaf_open(q0, p0, g0, q1, p1, eps, c, h):
        opened(q0, p0, g0, q1, p1, eps, c, h)
        qo, po = nc.oracle_open(q0, p0, g0, eps, c, h, dt)
        Bp = hc.p_bound(p0, g0, eps, h / 2, dt)
        worst[0] = max(worst[0], hc.ratio(hc._ld(p1) - po, Bp))
        worst[1] = max(worst[1], hc.ratio(hc._ld(q1) - qo, hc.q_bound(q0, po, Bp, eps, c, h, dt)))

    def leaf_close(q1, p1, g1, eps, c, h, q_far, p_far, out, ws=None):
        before = p1.clone()
        closed(q1, p1, g1, eps, c, h, q_far, p_far, out, ws)
        po, (E, far, near) = nc.oracle_close(q1, before, g1, eps, c, h, q_far, p_far, dt)
        Bp = hc.p_bound(before, g1, eps, h / 2, dt)
        B = (hc.energy_bound(po, Bp, c, dt, float(E)),) + nc.dots_bound(q1, q_far, p_far, po, Bp, dt)
        worst[2] = max(worst[2], hc.ratio(hc._ld(p1) - po, Bp))
        got = out.tolist()
        assert all(nc.within(o, w, b) for o, w, b in zip(got, (E, far, near), B)), (got, (E, far, near), B)
        worst[3] = max(worst[3], abs(got[0] - float(E)) / B[0])
        worst[4] = max(worst[4], max(abs(got[1] - float(far)) / B[1], abs(got[2] - float(near)) / B[2]))

    monkeypatch.setattr(nuts, 'leaf_open', leaf_open)
    monkeypatch.setattr(nuts, 'leaf_close', leaf_close)
    s.step()
    print('float32 leaves: worst error / bound  p(open) %.3f  q %.3f  p(close) %.3f  energy %.3f  projections %.3f' % tuple(worst))
    assert s.launches == 2 * (s.fn_evals - 1) + 1 and s.fn_evals > 3 and worst.max() <= 1.0
    assert all(v.dtype == dt for v in s.x.values())


def test_potential_backed_move_leaves_the_model_at_the_chain(monkeypatch):
    """Potential over a LogProb on the smallest RIME fixture (7 antennas, 10 point sources): after an accepted move the model
    stands at the proposal (not at the last leaf evaluated), after a rejected one back at the chain's position"""
    from bayeslim_amd import sky_model, beam_model, rime_model, optim, dataset, utils, telescope_model, sampler, nuts
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
        name = prob.named_params[0]
        pot = sampler.Potential(prob)
        x0 = ParamDict({name: prob[name].detach().clone()})
        scale = float(x0[name].abs().mean())
        np.random.seed(3)
        torch.manual_seed(3)
        s = nuts.NUTS(pot, x0, 1e-6 * scale, max_tree_depth=2)
        accept, p_acc = s.step()
        assert bool(accept) and float(p_acc) > 0.99 and s.fn_evals == 1 + 3 and s.launches == 1 + 2 * 3
        assert torch.equal(prob[name].detach(), s.x[name]) and isinstance(prob[name], torch.nn.Parameter)
        assert abs(float(s._U) - float(prob.closure())) <= 1e-12 * abs(float(s._U))
        x1 = s.x[name].clone()
        monkeypatch.setattr(np.random, 'rand', lambda: 2.0)                   # a draw no probability exceeds: forward, keep, reject
        s.eps = 1e-4 * scale
        accept, _ = s.step()
        assert not bool(accept) and s.fn_evals > 1 + 3
        assert torch.equal(s.x[name], x1) and torch.equal(prob[name].detach(), x1)
    finally:
        torch.set_default_dtype(old)
