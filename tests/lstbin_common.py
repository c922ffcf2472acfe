"""
Shared by tests/test_lstbin_host.py, tests/test_lstbin_gpu.py and tests/golden/make_golden_lstbin.py: the fixture loader of
tests/golden/lstbin.npz, the case tables the generator and the tests walk together, and a plain float64 numpy restatement
of rime_vis_timeavg_fwd / rime_vis_timeavg_bwd (csrc/lstbin.hip): over the members m of bin k in table order, t = members[m],

    sum_w    = sum w[t]                              avg     = sum w[t] V[t] exp(2 pi i nu tau[b, j]) / max(sum_w, 1e-40)
    avg_cov  = sum w[t]^2 cov[t] / max(sum_w, 1e-40)^2         avg_flag = every member flagged
    gV[t]    = sum_{m holding t} w[t] conj(phasor) g[k(m)] / max(sum_w[k(m)], 1e-40)

with j = t, or j = m when tau has one column per table position (by_member).

Kernel layout constants (csrc/lstbin.hip): a lane owns LANE_F[dtype] = 16 / sizeof(T) consecutive channels, a work-group of
256 lanes GROUP_F[dtype] = 256 LANE_F channels; NF lists 1 and width - 1, width, width + 1 of both.  With Nf below the
work-group width a work-group spans several rows, and with Nbl * Nbin * ... rows there is more than one work-group.

RESTATEMENT (measured against the REFERENCE's recorded outputs, never against the GPU code): the largest relative
discrepancy max|x - x_ref| / max|x_ref| of this restatement, fed with the recorded inputs, against every recorded output of
tests/golden/lstbin.npz (phasors, averaged data, cov, icov).  The restatement and the reference differ by rounding order
only (the reference multiplies by the phasor, then by the weight, and divides once), so the tests assert at FACTOR times it.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lstbin.npz')
_CACHE = {}

FACTOR = 100.0
# measured 2026-10-19 (x86-64 CPU, numpy float64) against tests/golden/lstbin.npz; set by the phasor of the vis_rephase case
# 'wide' (the reference exponentiates the unreduced phase of up to 56 turns); the next: time_nn_interp nn_wrap data 8.1e-15,
# lst_rephase per_time data 7.5e-15; every averaged cov / icov / time below 2e-15; flags equal
RESTATEMENT = 3.77e-14
TAU_RTOL = 1e-14             # tau against the recorded values (the issue's bound)

C_LIGHT = 2.99792458e8
SDAY_SEC = 86164.0905

# ------------------------------------------------------------------------------------------------- kernel case tables
LANE_F = {'f32': 4, 'f64': 2}
GROUP_F = {k: 256 * v for k, v in LANE_F.items()}
NF = {k: sorted({1, LANE_F[k] - 1, LANE_F[k], LANE_F[k] + 1, GROUP_F[k] - 1, GROUP_F[k], GROUP_F[k] + 1}) for k in LANE_F}
NPP = (1, 4)
NBL, NT = 3, 7
BIN_TABLES = {
    'full': [[0], [1, 2], [3, 4, 5, 6]],
    'dropped': [[0], [1, 2], [3, 5, 6]],                    # time 4 in no bin
    'repeated': [[0, 1], [1, 2], [3, 4, 5, 6, 3]],          # time 1 in two bins, time 3 twice in one
    'singleton': [[2], [0], [6], [6], [3]],                 # a gather (time_nn_interp): time 6 serves two bins
}
# (weights, cov, flags, rephasing)
OPTIONS = [(w, c, f, r) for w in (False, True) for c in (False, True) for f in (False, True) for r in (False, True)]
TOL_FWD = {'f32': 1e-5, 'f64': 1e-12}                       # of max|V|: the visibility tolerances of the README
TOL_BWD = {'f32': 1e-4, 'f64': 1e-10}                       # of the maximum

# ------------------------------------------------------------------------------------------------- fixture case tables
# the public interface: 3 baselines of a 4-antenna layout, 7 times 5 minutes apart, 5 channels
FIX_NF, FIX_NT = 5, 7
FIX_LAT, FIX_LON = -30.72148, 21.42827
FIX_JD0, FIX_DT = 2459861.3, 5.0 / 1440
FIX_ANTS = [0, 1, 2, 3]
FIX_ANTVECS = [[0.0, 0.0, 0.0], [14.6, 0.0, 0.0], [7.3, 12.6, 0.1], [-30.0, 41.0, -0.2]]
FIX_BLS = [(0, 1), (0, 2), (1, 3)]
FIX_FREQS = np.linspace(120e6, 180e6, FIX_NF)
# vis_rephase: name -> (dlst [rad], lat [deg])
REPHASE_CASES = {
    'scalar': (np.array(0.01), FIX_LAT),
    'zero': (np.zeros(3), FIX_LAT),
    'ramp': (np.linspace(-0.05, 0.05, FIX_NT), FIX_LAT),
    'equator': (np.linspace(-0.3, 0.3, 4), 0.0),
    'wide': (np.array([-1.0, 0.5, 2.0]), 45.0),
}
# time_average: name -> (pol, time_inds, weights from icov, cov set, flags, rephase)
AVG_CASES = {
    'all_plain': (None, None, False, False, False, False),
    'bins_icov': (None, [[0], [1, 2], [3, 4, 5, 6]], True, False, True, False),
    'bins_cov': ('ee', [[0], [1, 2], [3, 4, 5, 6]], True, True, True, False),
    'dropped': ('ee', [[0], [1, 2], [3, 5, 6]], True, True, False, False),     # the reference raises with flags AND dropped times
    'rephase_plain': ('ee', [[0, 1, 2], [3, 4, 5, 6]], False, False, False, True),
    'rephase_icov': (None, [[0, 1], [2, 3, 4], [5, 6]], True, True, True, True),
    'rephase_dropped': ('ee', [[1, 2], [4, 5, 6]], True, False, True, True),
}
# lst_rephase: name -> (pol, dLST)
LSTR_CASES = {
    'scalar': ('ee', np.array(0.02)),
    'per_time': (None, np.linspace(-0.03, 0.04, FIX_NT)),
}
# time_nn_interp: name -> (pol, first JD of the data, target LSTs as offsets [rad] from the LST of the first time, rephase)
_STEP = 2 * np.pi * FIX_DT * 86400.0 / SDAY_SEC             # LST step of one integration
NN_CASES = {
    'nn_grid': (None, FIX_JD0, np.array([0.2, 1.4, 1.6, 3.3, 5.9]) * _STEP, True),
    'nn_fine': ('ee', FIX_JD0, np.arange(0.0, 3.0, 0.4) * _STEP, True),          # integrations serve several targets
    'nn_norephase': ('ee', FIX_JD0, np.array([0.9, 2.2, 4.6]) * _STEP, False),
    'nn_wrap': ('ee', None, np.array([0.3, 1.7, 3.1, 4.4, 5.8]) * _STEP, True),   # the data cross LST = 2 pi (JD chosen so)
}


def jd2lst(jd, longitude):
    """LST [deg] as a linear function of the Julian date: the stand-in for JD2LST under which the time_nn_interp records
    were made (the reference's needs astropy) and under which the tests compare"""
    return (100.0 + 360.0 * 86400.0 / SDAY_SEC * (np.asarray(jd, dtype=np.float64) - 2459861.0) + longitude) % 360.0


def wrap_jd0():
    """first JD of a 7-integration block whose LST passes 2 pi between its third and fourth time"""
    lst0 = jd2lst(FIX_JD0, FIX_LON)
    return FIX_JD0 + ((360.0 - lst0) / 360.0 * SDAY_SEC / 86400.0) - 2.5 * FIX_DT


def fix_times(jd0):
    """the 7 Julian dates of a case (jd0 None: the block that crosses LST = 2 pi)"""
    return (wrap_jd0() if jd0 is None else jd0) + np.arange(FIX_NT) * FIX_DT


def fix_inputs(name, pol):
    """(data, icov, cov, flags) of a public-interface case: float64 / complex128, seeded by the case name"""
    rng = np.random.default_rng(sum(name.encode()) + 7)
    shape = ((2, 2) if pol is None else (1, 1)) + (len(FIX_BLS), FIX_NT, FIX_NF)
    data = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    icov = rng.uniform(0.5, 2.0, size=shape)
    flags = rng.uniform(size=shape) < 0.4
    flags[..., 0, :2, :] = True                              # bins whose members are all flagged exist
    return data, icov, 1 / icov, flags


def golden():
    """lstbin.npz as a dict of numpy arrays, loaded once and never modified by a test"""
    if GOLDEN not in _CACHE:
        with np.load(GOLDEN) as f:
            _CACHE[GOLDEN] = {k: f[k] for k in f.files}
    return _CACHE[GOLDEN]


# ------------------------------------------------------------------------------------------------- restatement of the kernel
def tau_of(dlst, lat, blvecs):
    """float64 restatement of telescope_model.rephase_tau: (Nbl, Nlst)"""
    H = -np.atleast_1d(np.asarray(dlst, dtype=np.float64))
    d = np.deg2rad(lat)
    top2eq_z = np.array([np.cos(d), 0.0, np.sin(d)])
    out = []
    for h in H:
        eq2top = np.array([[np.sin(h), np.cos(h), 0.0],
                           [-np.sin(d) * np.cos(h), np.sin(d) * np.sin(h), np.cos(d)],
                           [np.cos(d) * np.cos(h), -np.cos(d) * np.sin(h), np.sin(d)]])
        out.append(np.asarray(blvecs, dtype=np.float64) @ (eq2top @ top2eq_z - np.array([0.0, 0.0, 1.0])) / C_LIGHT)
    return np.stack(out, axis=1)


def csr(bins):
    """(bin_ptr, members) of a list of bins"""
    ptr = np.zeros(len(bins) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(b) for b in bins])
    mem = np.concatenate([np.asarray(b, dtype=np.int64).reshape(-1) for b in bins]) if len(bins) else np.zeros(0, dtype=np.int64)
    return ptr, mem.astype(np.int64)


def transpose(bins, Nt):
    """for every time, the (table position, bin) pairs that hold it, ascending position: a plain double loop"""
    out = [[] for _ in range(Nt)]
    m = 0
    for k, b in enumerate(bins):
        for t in b:
            out[int(t)].append((m, k))
            m += 1
    return out


def phasor(tau, freqs):
    """exp(2 pi i nu tau) with the phase reduced to a fraction of a turn first: tau (...,) -> (..., Nf)"""
    ph = np.asarray(tau, dtype=np.float64)[..., None] * np.asarray(freqs, dtype=np.float64)
    return np.exp(2j * np.pi * (ph - np.rint(ph)))


def timeavg(data, bins, wgts=None, cov=None, flags=None, tau=None, freqs=None, by_member=False, shape=None):
    """(avg, sum_w, avg_cov, avg_flag) in float64 / complex128; data (..., Nbl, Nt, Nf) or None with `shape`"""
    shape = tuple(data.shape) if data is not None else tuple(shape)
    Nf = shape[-1]
    oshape = shape[:-2] + (len(bins), Nf)
    avg, sum_w = np.zeros(oshape, dtype=np.complex128), np.zeros(oshape)
    avg_cov = np.zeros(oshape) if cov is not None else None
    avg_flag = np.ones(oshape, dtype=bool) if flags is not None else None
    m = 0
    for k, b in enumerate(bins):
        for t in b:
            t = int(t)
            v = np.asarray(data[..., t, :], dtype=np.complex128) if data is not None else np.ones(shape[:-2] + (Nf,), dtype=np.complex128)
            w = np.asarray(np.broadcast_to(wgts, shape)[..., t, :], dtype=np.float64) if wgts is not None else np.ones(v.shape)
            if tau is not None:
                v = v * phasor(np.asarray(tau)[:, m if by_member else t], freqs)
            avg[..., k, :] += w * v
            sum_w[..., k, :] += w
            if cov is not None:
                avg_cov[..., k, :] += w ** 2 * np.broadcast_to(cov, shape)[..., t, :]
            if flags is not None:
                avg_flag[..., k, :] &= np.broadcast_to(flags, shape)[..., t, :]
            m += 1
    d = np.maximum(sum_w, 1e-40)
    return avg / d, sum_w, (avg_cov / d ** 2 if cov is not None else None), avg_flag


def timeavg_adjoint(g, bins, Nt, sum_w, wgts=None, tau=None, freqs=None, by_member=False):
    """gV (..., Nbl, Nt, Nf) of g (..., Nbl, Nbin, Nf): the adjoint of timeavg with respect to the data, float64"""
    shape = tuple(g.shape[:-2]) + (Nt, g.shape[-1])
    gv = np.zeros(shape, dtype=np.complex128)
    d = np.maximum(np.asarray(sum_w, dtype=np.float64), 1e-40)
    for t, lst in enumerate(transpose(bins, Nt)):
        w = np.asarray(np.broadcast_to(wgts, shape)[..., t, :], dtype=np.float64) if wgts is not None else 1.0
        for m, k in lst:
            x = np.asarray(g[..., k, :], dtype=np.complex128) / d[..., k, :]
            if tau is not None:
                x = x * np.conj(phasor(np.asarray(tau)[:, m if by_member else t], freqs))
            gv[..., t, :] += w * x
    return gv


def rel_err(x, ref):
    ref = np.asarray(ref)
    scale = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(np.asarray(x) - ref).max() if ref.size else 0.0
    return err / scale if scale > 0 else err


# ------------------------------------------------------------------------------------- the fixture cases, restated in float64
def fix_blvecs():
    v = np.asarray(FIX_ANTVECS)
    return np.stack([v[FIX_ANTS.index(j)] - v[FIX_ANTS.index(i)] for i, j in FIX_BLS])


def nearest(lsts, self_lsts):
    """(t_idx, dLST): the nearest data LST of every target after unwrapping both sets across 2 pi, as plain loops"""
    lsts, self_lsts = [float(x) for x in lsts], [float(x) for x in self_lsts]
    if lsts[-1] < lsts[0]:
        lsts = [x + 2 * np.pi if x < lsts[0] else x for x in lsts]
    if self_lsts[-1] < self_lsts[0]:
        self_lsts = [x + 2 * np.pi if x < self_lsts[0] else x for x in self_lsts]
    if lsts[0] < self_lsts[0]:
        lsts = [x + 2 * np.pi for x in lsts]
    idx = [min(range(len(self_lsts)), key=lambda j: (abs(self_lsts[j] - x), j)) for x in lsts]
    return np.array(idx), np.array([x - self_lsts[j] for x, j in zip(lsts, idx)])


def restate_case(kind, name):
    """dict of the outputs (data, times, flags, cov, icov as recorded) of one fixture case from its recorded inputs"""
    G = golden()
    bv = G['blvecs']
    if kind == 'rephase':
        dlst, lat = REPHASE_CASES[name]
        tau = tau_of(dlst, lat, bv)
        return {'tau': tau, 'phasor': phasor(tau, FIX_FREQS)}
    if kind == 'lstr':
        pol, dlst = LSTR_CASES[name]
        tau = tau_of(np.broadcast_to(dlst, (FIX_NT,)), FIX_LAT, bv)
        data = timeavg(G['lstr_%s_data' % name], [[t] for t in range(FIX_NT)], tau=tau, freqs=FIX_FREQS)[0]
        return {'data': data, 'times': fix_times(FIX_JD0)}
    if kind == 'nn':
        pol, jd0, offs, rephase = NN_CASES[name]
        times, lsts = G[name + '_times'], G[name + '_lsts']
        t_idx, dLST = nearest(lsts, np.deg2rad(jd2lst(times, FIX_LON)))
        tau = tau_of(dLST, FIX_LAT, bv) if rephase else None
        data, _, cov, flags = timeavg(G[name + '_data'], [[t] for t in t_idx], cov=G[name + '_cov'], flags=G[name + '_flags'],
                                      tau=tau, freqs=FIX_FREQS, by_member=True)
        return {'data': data, 'times': times[t_idx], 'flags': flags, 'cov': cov, 'icov': G[name + '_icov'][..., t_idx, :]}
    pol, time_inds, use_icov, use_cov, use_flags, rephase = AVG_CASES[name]
    key = 'avg_' + name
    times = G[key + '_times']
    bins = [list(range(FIX_NT))] if time_inds is None else time_inds
    icov, cov, flags = G.get(key + '_icov'), G.get(key + '_cov'), G.get(key + '_flags')
    avg_times = np.array([times[b].mean() for b in bins])
    tau = None
    if rephase:
        dl = np.zeros(FIX_NT)
        for k, b in enumerate(bins):
            dl[b] = (avg_times[k] - times[b]) * 2 * np.pi / (SDAY_SEC / 86400.0)
        tau = tau_of(dl, FIX_LAT, bv)
    cv = cov if cov is not None else (1 / np.maximum(icov, 1e-60) if icov is not None else None)
    data, _, avg_cov, avg_flags = timeavg(G[key + '_data'], bins, wgts=icov, cov=cv, flags=flags, tau=tau, freqs=FIX_FREQS)
    out = {'data': data, 'times': avg_times}
    if flags is not None:
        out['flags'] = avg_flags
    if icov is not None:
        out['icov'] = 1 / np.maximum(avg_cov, 1e-60)
    if cov is not None:
        out['cov'] = avg_cov
    return out


def fixture_cases():
    return ([('lstr', n) for n in LSTR_CASES] + [('nn', n) for n in NN_CASES] + [('avg', n) for n in AVG_CASES])


def recorded(kind, name):
    """the recorded outputs of a case, keyed as restate_case keys them"""
    G = golden()
    if kind == 'rephase':
        return {'tau': G['rephase_%s_tau' % name], 'phasor': G['rephase_%s_phasor' % name]}
    prefix = (name if kind == 'nn' else kind + '_' + name) + '_out_'
    return {k[len(prefix):]: v for k, v in G.items() if k.startswith(prefix)}


def compare(got, ref, tol_of):
    """assert every recorded output: booleans equal, numbers within tol_of(key) relative to the largest recorded magnitude;
    returns the largest relative discrepancy per key"""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = {}
    for k, r in ref.items():
        g = np.asarray(got[k])
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if r.dtype == bool:
            assert g.dtype == bool and (g == r).all(), k
            continue
        worst[k] = rel_err(g, r)
        assert worst[k] <= tol_of(k), (k, worst[k], tol_of(k))
    return worst
