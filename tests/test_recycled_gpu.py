"""
GPU checks of csrc/recycle.hip and of bayeslim_amd/recycled.py on it: the bit contract of rime_hmc_recycle against the three-call
composition (rime_hmc_step with the energy, two copies, rime_hmc_step) at the shapes of recycled_common, with every vector in turn
off a 16-byte boundary and eps / c null and present; the kernel against the numpy restatement within the bounds of hmc_common; the
seeded chains of tests/golden/recycled.npz in both precisions; the launch count; the chain entries of the one-copy path;
recycled.HMC against sampler.HMC bit for bit; the dynamic step size after every kind of move; the momentum masks; estimate_cov.
"""
import numpy as np
import pytest
import torch

import hmc_common as hc
import recycled_common as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = (torch.float32, torch.float64)
NAMES = ('q', 'p', 'g', 'eps', 'c', 'q_out', 'p_out')
HALF, DRIFT = 0.5 * 0.37, 0.37                     # a step folded into the flags: T(half) is a rounding of its own in float32
SENTINEL = -7.25


def operands(rng, N, dtype, shift=None):
    """the seven vectors, each with one spare element after it (the sentinel) and `shift` one element off a 16-byte boundary"""
    out = {}
    for name in NAMES:
        x = rng.uniform(0.5, 2.0, N) if name in ('eps', 'c') else rng.normal(size=N)
        off = 4 + (1 if name == shift else 0)       # 4 elements keep either precision on a 16-byte boundary
        buf = torch.full((N + off + 1,), SENTINEL, dtype=dtype, device=DEV)
        buf[off:off + N] = torch.as_tensor(x).to(dtype)
        out[name] = buf[off:off + N]
        out['_' + name] = buf
        assert (out[name].data_ptr() % 16 != 0) == (name == shift)
    return out


def composition(o, eps, c, drift):
    """the bit contract's right-hand side on clones: (q, p, q_out, p_out, energy)"""
    from bayeslim_amd import sampler
    q, p = o['q'].clone(), o['p'].clone()
    e = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV)
    sampler.hmc_step(None, p, o['g'], eps, c, HALF, 0.0, e)
    q_out, p_out = q.clone(), p.clone()
    if drift:
        sampler.hmc_step(q, p, o['g'], eps, c, HALF, drift)
    return q, p, q_out, p_out, float(e)


def fused(o, eps, c, drift):
    from bayeslim_amd import recycled
    e = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV)
    recycled.hmc_recycle(o['q'], o['p'], o['g'], eps, c, HALF, drift, o['q_out'], o['p_out'], e)
    return o['q'], o['p'], o['q_out'], o['p_out'], float(e)


def assert_nothing_at_zero(dtype, with_eps, with_c, drift):
    """N = 0 through the library itself (an empty tensor has no address to hand over): nothing is written but energy = 0, which
    is rime_hmc_step's"""
    from bayeslim_amd import _lib
    from bayeslim_amd.ops import _ptr, _stream
    v = {n: torch.full((1,), SENTINEL, dtype=dtype, device=DEV) for n in NAMES}
    ws = torch.zeros(1, dtype=torch.float64, device=DEV)
    e = [torch.full((1,), float('nan'), dtype=torch.float64, device=DEV) for _ in range(2)]
    code = 0 if dtype == torch.float32 else 1
    eps, c = (v['eps'] if with_eps else None), (v['c'] if with_c else None)
    assert _lib.lib.rime_hmc_recycle(code, 0, _ptr(v['q']), _ptr(v['p']), _ptr(v['g']), _ptr(eps), _ptr(c), HALF, drift, _ptr(v['q_out']),
                                     _ptr(v['p_out']), _ptr(e[0]), _ptr(ws), 8, _stream()) == 0
    assert _lib.lib.rime_hmc_step(code, 0, None, _ptr(v['p']), _ptr(v['g']), _ptr(eps), _ptr(c), HALF, 0.0, _ptr(e[1]), _ptr(ws), 8,
                                  _stream()) == 0
    assert float(e[0]) == float(e[1]) == 0.0 and all(float(t) == SENTINEL for t in v.values())


def assert_contract(rng, N, dtype, shift, with_eps, with_c, drift):
    if N == 0:
        return assert_nothing_at_zero(dtype, with_eps, with_c, drift)
    o = operands(rng, N, dtype, shift)
    eps, c = (o['eps'] if with_eps else None), (o['c'] if with_c else None)
    want = composition(o, eps, c, drift)
    g0, e0, c0 = o['g'].clone(), o['eps'].clone(), o['c'].clone()
    got = fused(o, eps, c, drift)
    what = (N, dtype, shift, with_eps, with_c, drift)
    for name, a, b in zip(('q', 'p', 'q_out', 'p_out'), got, want):
        assert torch.equal(a, b), (name,) + what
    assert got[4] == want[4] and (np.isfinite(got[4]) if N else got[4] == 0.0), what
    assert torch.equal(o['g'], g0) and torch.equal(o['eps'], e0) and torch.equal(o['c'], c0)
    for name in NAMES:                              # nothing before the vector, nothing past N
        buf = o['_' + name]
        assert float(buf[-1]) == SENTINEL and bool((buf[:buf.numel() - 1 - N] == SENTINEL).all()), (name,) + what
    if N and drift:
        assert not torch.equal(got[0], got[2]) and not torch.equal(got[1], got[3])


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_bit_contract_over_sizes_and_nulls(dtype):
    rng = np.random.default_rng(31)
    for N in rc.KERNEL_NS:
        for with_eps, with_c in ((False, False), (True, False), (False, True), (True, True)):
            for drift in (0.0, DRIFT):
                assert_contract(rng, N, dtype, None, with_eps, with_c, drift)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_bit_contract_with_each_vector_misaligned(dtype):
    rng = np.random.default_rng(32)
    for N in (65, 4097):
        for shift in NAMES:
            for drift in (0.0, DRIFT):
                assert_contract(rng, N, dtype, shift, True, True, drift)
        assert_contract(rng, N, dtype, 'q', False, False, DRIFT)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_bit_contract_beyond_the_largest_grid(dtype):
    """more than STEP_MAXBLOCKS chunks plus a chunk and a tail: some work-groups take a second trip of the grid-stride loop"""
    from bayeslim_amd import sampler
    rng = np.random.default_rng(33)
    N = rc.second_trip_N(sampler.STEP_MAXBLOCKS, sampler.STEP_SPAN[dtype])
    assert_contract(rng, N, dtype, None, True, True, DRIFT)
    assert_contract(rng, N, dtype, 'p_out', False, True, 0.0)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_kernel_against_the_oracle(dtype):
    rng = np.random.default_rng(34)
    N = rc.ORACLE_N
    worst = np.zeros(4)
    for with_eps, with_c, drift in ((True, True, DRIFT), (False, False, DRIFT), (True, True, 0.0)):
        o = operands(rng, N, dtype)
        eps, c = (o['eps'] if with_eps else None), (o['c'] if with_c else None)
        q2, p2, qo, po, E, (Bq, Bp, Bpo, BE) = rc.oracle_recycle(o['q'], o['p'], o['g'], eps, c, HALF, drift, dtype)
        got = fused(o, eps, c, drift)
        r = (hc.ratio(hc._ld(got[0]) - q2, Bq), hc.ratio(hc._ld(got[1]) - p2, Bp), hc.ratio(hc._ld(got[3]) - po, Bpo),
             abs(got[4] - float(E)) / BE)
        assert np.array_equal(hc._ld(got[2]), qo)
        worst = np.maximum(worst, r)
        assert max(r) <= 1.0, (with_eps, with_c, drift, r)
    print('%s: worst error / bound  q %.3f  p %.3f  p_out %.3f  energy %.3f' % (dtype, *worst))


# ----------------------------------------------------------------------------------------------------- the samplers
def to_dev(d, dtype):
    cd = torch.complex64 if dtype == torch.float32 else torch.complex128
    return {k: torch.tensor(v, device=DEV).to(cd if np.iscomplexobj(v) else dtype) for k, v in d.items()}


def make(cls, g, tag, dtype, keys=rc.KEYS, **kw):
    """a sampler of bayeslim_amd on the inputs of chain `tag`"""
    from bayeslim_amd import recycled
    from bayeslim_amd.paramdict import ParamDict
    a, x0, cov, hess, draws, eps, pmask, dyn, dHmax = rc.chain_setup(g, tag)
    sub = lambda d: {k: d[k] for k in keys}
    a, x0, cov, hess, draws = [to_dev(sub(d), dtype) for d in (a, x0, cov, hess, draws)]

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

    e = to_dev({k: np.asarray(eps[k]) for k in keys}, dtype)
    if tag == 'b':
        e = recycled.StepSize(e)
    elif tag == 'c':
        e = recycled.DynamicStepSize(e, **dyn)
    else:
        e = ParamDict(e)
    if pmask is not None:                           # chain d: the recorded masks, None where the reference was given ones
        m = to_dev({k: pmask[k] for k in keys}, dtype)
        kw.setdefault('pmask', {k: (None if k == 'v' else m[k]) for k in keys})
    kw.setdefault('dHmax', dHmax)
    kw.setdefault('Nstep', rc.NSTEP)
    return cls(potential, ParamDict(x0), e, cov_L=ParamDict(cov), hess_L=ParamDict(hess), pdist={k: dist(k) for k in x0}, **kw)


def run_chain(g, tag, dtype):
    from bayeslim_amd import recycled
    np.random.seed(rc.CHAINS[tag]['seed'])
    s = make(recycled.RecycledHMC, g, tag, dtype, record_divergences=True)
    recs = []
    for _ in range(rc.MOVES):
        n_acc, launches, evals = len(s._acceptances), s._traj.launches, s.fn_evals
        accept, prob = s.step()
        H = s._last['H']
        div = len(s._acceptances) == n_acc
        if not div:
            # fused: the starting energy, the opening stage, Nstep recycle launches; masked (chain d): per step the closing kick,
            # the energy pass and, but on the last step, the opening stage
            assert s._traj.launches == launches + (3 * rc.NSTEP + 1 if tag == 'd' else rc.NSTEP + 2)
            assert s.fn_evals == evals + rc.NSTEP
            assert bool(accept) == s._acceptances[-1]
        else:
            assert not bool(accept) and float(prob) == 0.0 and len(H) <= rc.NSTEP
        recs.append(dict(H_start=s._last['H_start'], H=H, accept=s._acceptances[n_acc:], div=div, prob=float(prob), U=float(s._U),
                         nchain=len(s.Uchain), x={k: s.x[k].cpu().numpy() for k in rc.KEYS},
                         eps_mul={k: float(v) for k, v in s.eps.eps_mul.items()} if tag == 'c' else None))
    return s, recs


@pytest.mark.parametrize('tag', rc.TAGS)
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_seeded_chain_against_the_reference(tag, dtype):
    """the reference's decisions in both precisions; in float64 its energies, positions and potentials within TOL_CHAIN"""
    g = rc.golden()
    s, recs = run_chain(g, tag, dtype)
    assert rc.same_decisions(recs, g, tag), (rc.decisions(recs), g[tag + '_accept'], g[tag + '_div'], g[tag + '_nchain'])
    if tag == 'c':
        assert np.array_equal(rc.eps_mul_of(recs), g['c_eps_mul'])
    if tag == 'e':
        assert len(s._divergences) == int(g['e_div'].sum()) and s._divergences[0][1]['u'].shape == hc.SHAPES['u']
    if dtype == torch.float64:
        e = rc.chain_discrepancy(recs, g, tag)
        print('chain %s on the GPU: %.3e' % (tag, e))
        assert e <= rc.TOL_CHAIN
    assert len(s.Uchain) == int(g[tag + '_nchain'][-1]) and len(s.chain['w']) == len(s.Uchain)
    assert s.chain['w'][0].dtype == (np.complex64 if dtype == torch.float32 else np.complex128)


def test_chain_entries_are_those_of_append_chain():
    """the one-copy path against SamplerBase.append_chain on the same rows: array for array, dtype, shape and order"""
    from bayeslim_amd import recycled, sampler
    g = rc.golden()
    np.random.seed(rc.CHAINS['b']['seed'])
    s = make(recycled.RecycledHMC, g, 'b', torch.float64)
    ref = sampler.SamplerBase(s.x)
    for _ in range(rc.MOVES - 1):                   # move 4 of chain b refuses its second state: rows that are not a range
        n = len(s._acceptances)
        s.step()
        for i, acc in enumerate(s._acceptances[n:]):
            if acc:
                ref.append_chain(s._lay.views(s._rows_q[i, :s._lay.N]), U=None)
    assert len(ref.Uchain) == len(s.Uchain) > rc.NSTEP and not all(s._acceptances)
    for k in rc.KEYS:
        for got, want in zip(s.chain[k], ref.chain[k]):
            assert type(got) is type(want) and got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(s.chain['u'][-1], s.x['u'].cpu().numpy())
    s.sample(1)
    assert s.accept_ratio == sum(s._acceptances) / len(s._acceptances) and len(s._acceptances) == rc.MOVES * rc.NSTEP


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_hmc_with_a_plain_step_is_sampler_hmc_bit_for_bit(dtype):
    from bayeslim_amd import recycled, sampler
    g = rc.golden()
    out = []
    for cls in (sampler.HMC, recycled.HMC):
        np.random.seed(7)
        s = make(cls, g, 'a', dtype)
        s.sample(4)
        out.append(s)
    a, b = out
    assert a._acceptances == b._acceptances and a._last == b._last and [float(u) for u in a.Uchain] == [float(u) for u in b.Uchain]
    assert all(torch.equal(a.x[k], b.x[k]) for k in rc.KEYS)
    assert all(np.array_equal(x, y) for k in rc.KEYS for x, y in zip(a.chain[k], b.chain[k]))
    assert any(a._acceptances)


def test_dynamic_stepsize_updates_after_every_kind_of_move():
    from bayeslim_amd import recycled
    g = rc.golden()
    np.random.seed(3)
    s = make(recycled.HMC, g, 'c', torch.float64, Nstep=3)
    mul = lambda: float(s.eps.eps_mul['u'])
    s.eps.eps_mul = {k: v * 0.25 for k, v in s.eps.eps_mul.items()}
    accept, prob = s.step()                                       # a short, well-resolved trajectory: accepted
    assert bool(accept) and float(prob) >= rc.DYN['min_prob'] and mul() == 0.5
    assert torch.equal(s._eps_flat, recycled.expand_eps(s._lay, s.eps)) and float(s._eps_flat[0]) == 0.5 * rc.EPS['u']
    s.append_chain(s.x, U=s._U)
    s.eps.params = {k: v * 40 for k, v in s.eps.params.items()}  # far too long a step: refused
    s.eps = s.eps
    s.dHmax = float('inf')                                        # (refused by the Metropolis test, not as a divergence)
    accept, prob = s.step()
    assert not bool(accept) and float(prob) < rc.DYN['min_prob'] and mul() == 0.25 and np.isfinite(s._last['H_end'])
    s.dHmax = 0.0                                                 # and now divergent: updated on that path too
    n = s._traj.launches
    accept, prob = s.step()
    assert not bool(accept) and float(prob) == 0.0 and s._last['H_end'] - s._last['H_start'] > 0 and mul() == 0.125
    assert s._traj.launches > n and torch.equal(s._eps_flat, recycled.expand_eps(s._lay, s.eps))
    assert float(s._eps_flat[0]) == float(s.eps['u'].reshape(-1)[0]) == float(s.eps.params['u'].reshape(-1)[0]) * 0.125


def test_momentum_masks():
    from bayeslim_amd import recycled
    g = rc.golden()
    mask = to_dev({k: g['in_mask_' + k] for k in rc.KEYS}, torch.float64)
    s = make(recycled.HMC, g, 'a', torch.float64, pmask={'u': mask['u'], 'v': None, 'w': mask['w']})
    hess, draw = to_dev({k: g['in_hess_' + k] for k in rc.KEYS}, torch.float64), to_dev({k: g['in_draws_' + k][0] for k in rc.KEYS}, torch.float64)
    p = s.draw_momentum()
    assert torch.equal(p['v'], hess['v'] * draw['v'])
    assert torch.equal(p['u'], mask['u'] * (hess['u'] * (draw['u'] * mask['u'])))
    want = recycled.multiply_eps(hess['w'] * recycled.multiply_eps(draw['w'], mask['w']), mask['w'])
    assert torch.equal(p['w'], want) and bool((p['w'].real[mask['w'].real == 0] == 0).all()) and bool((p['w'].imag != 0).any())
    assert bool((p['u'] == 0).any()) and bool((p['u'] != 0).any())
    ones = s.x.ones()
    assert s.apply_pmask(ones, inplace=False) is not ones and torch.equal(s.apply_pmask(ones)['u'], mask['u'])
    # one masked move against the float64 restatement (the mask in draw_momentum only): energies, probability, position
    K_start, H_start, H_end, prob, q = rc.oracle_hmc_move(g, rc.NSTEP)
    np.random.seed(1)
    s = make(recycled.HMC, g, 'a', torch.float64, pmask={'u': mask['u'], 'v': None, 'w': mask['w']})     # fresh: the first draws
    accept, got = s.step()
    scale = max(abs(H_start), abs(H_end))
    assert abs(s._last['K_start'] - K_start) <= rc.TOL_CHAIN * scale and abs(s._last['H_start'] - H_start) <= rc.TOL_CHAIN * scale
    assert abs(s._last['H_end'] - H_end) <= rc.TOL_CHAIN * scale and abs(float(got) - prob) <= 2 * rc.TOL_CHAIN * scale
    for k in rc.KEYS:
        assert np.abs(s._traj.qv[k].cpu().numpy() - q[k]).max() <= rc.TOL_CHAIN * np.abs(q[k]).max()
    # and the masks matter to it: the unmasked move ends elsewhere
    assert abs(rc.oracle_hmc_move(g, rc.NSTEP, masked=False)[2] - H_end) > 1e-3


def test_estimate_cov_sets_the_mass():
    from bayeslim_amd import recycled, massmat
    g = rc.golden()
    np.random.seed(5)
    s = make(recycled.HMC, g, 'a', torch.float64, keys=('u', 'v'), Nstep=2)
    s.sample(5)
    s.estimate_cov(Nback=5)
    for k in ('u', 'v'):
        want = np.sqrt(np.var(np.array(s.chain[k])[-5:], axis=0))
        assert np.array_equal(s.cov_L[k].cpu().numpy(), want) and s.cov_L[k].shape == hc.SHAPES[k]
        assert torch.equal(s.hess_L[k], 1 / s.cov_L[k])
    s.step()
    with pytest.raises(NotImplementedError, match='massmat'):
        s.estimate_cov(diag_mass=False)
    # the dense factor of the module function is what massmat.HMC.set_chol takes
    chain = {'v': [np.random.default_rng(i).normal(size=4) for i in range(30)]}
    L = recycled.estimate_cov(chain, diag_mass=False, eps={'v': 1e-6}, device=DEV)
    pot = lambda x: ((x['v'] ** 2).sum() / 2, x)
    from bayeslim_amd.paramdict import ParamDict
    m = massmat.HMC(pot, ParamDict({'v': torch.zeros(4, dtype=torch.float64, device=DEV)}), 0.1, cov_L=L, diag_mass=False, Nstep=2)
    m.set_chol(cov_L=L, diag_mass=False)
    accept, prob = m.step()
    assert 0.0 <= float(prob) <= 1.0
