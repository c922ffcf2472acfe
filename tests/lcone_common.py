"""
Shared by tests/test_lcone_host.py, tests/test_lcone_gpu.py and tests/golden/make_golden_lcone.py: the fixture loader of
tests/golden/lcone.npz, the case tables the generator and the tests walk together, a plain float64 numpy restatement of
rime_lcone_fwd (csrc/lcone.hip) in the kernel's operation order, and the error bound counted from that order.

Restatement.  Per (radius i, pixel p), position x = (v * dc) / sim_res per axis in float64 (PLANE: z = dc / sim_res alone),
    nearest:  i = rint(x) mod N                      linear:  i0 = floor(x) mod N,  i1 = (i0 + 1) mod N,  f = x - floor(x)
    source index (i - roll) mod N,
    lerp(a, b; f) = a (1 - f) + b f  along x, then y, then z;   out = sum_s w[i, s] val_s  in ascending s.

BOUND.  The output is  sum_s w_s sum_corners omega_c v_c  with omega >= 0 and sum omega = 1, so every intermediate of the
kernel is bounded by W M (1 + O(eps)), W = sum_s |w_s| of the radius, M = max|cube|.  The kernel (T the cube dtype, eps_T its
machine epsilon, every rounding at most eps_T / 2 relative) rounds, on the longest path from a voxel to the output:
    linear, sphere:  3 fractions f to T (each moves the result by at most |b - a| eps_T / 2 <= M eps_T), 3 complements
                     g = 1 - f, and per lerp level one product a g and one fma: 3 + 3 + 3 x 2 = 12
    linear, plane:   1 + 1 + 2 = 4                      nearest: 0
    radial:          the weight to T (1), one product and S - 1 fmas (S): 1 + S
so K = K_spatial + 1 + S, and |kernel - exact| <= K eps_T W M per radius: each of the K roundings is counted at a full
eps_T W M, twice what all but the fractions can contribute, which covers the second-order terms ((1 + eps_T / 2)^16 - 1 -
8 eps_T is below 1e-12 eps_T).  The float64 restatement differs from the exact value by the same count at eps of float64,
added in.  Derived here, never tuned to a GPU result; it scales with the extrapolation weights by construction.

RESTATEMENT (measured against the REFERENCE's recorded outputs, never against the GPU code): the largest relative
discrepancy max|x - x_ref| / max|x_ref| of the restatement, fed with the recorded inputs, over every pinned case of
tests/golden/lcone.npz.  The reference forms b r + c per voxel with cancellation of order r / dr; the restatement weights
the samples.  The tests assert at FACTOR times it.  'quadratic' is recorded for information only (the reference's branch is
not the parabola through its cubes: cosmology.cube2lcone, deviation 1).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lcone.npz')
_CACHE = {}

FACTOR = 100.0
# measured 2026-10-20 (x86-64 CPU, numpy float64) against tests/golden/lcone.npz over all 36 pinned cases; set by the linear
# radial cases (the reference's b r + c cancels to r / dr ~ 1500 eps; worst: desc_linear_linear_roll0 2.22e-13, the next
# desc_linear_nearest_roll0 1.97e-13, asc_linear_linear_roll0 1.66e-13); all 20 'nearest' radial cases: 0 (bit-equal)
RESTATEMENT = 2.3e-13

# ------------------------------------------------------------------------------------------------------- case tables
EXT = (5, 6, 7)                       # unequal, so that a swapped stride shows
NSIM = 4
SIM_R = {'asc': np.array([8990.0, 8996.0, 9005.0, 9012.5])}          # ascending, unevenly spaced
SIM_R['desc'] = SIM_R['asc'][::-1].copy()
SIM_RES = 2.0                         # dc / sim_res ~ 4500 >> N: a shell wraps hundreds of times
# below the range, on a node, between nodes, exactly midway between two nodes, near the top, above the range
R = np.array([8985.5, 8996.0, 8999.3, 9000.5, 9011.9, 9016.7])
ROLLS = [None, 3, (1, 0, -2), (-9, 13, 7)]
NPIX = (1, 63, 64, 65, 255, 256, 257)
NR = (1, 2, 6)
RINTERP = ('nearest', 'linear', 'quadratic')
INTERP = ('nearest', 'linear')
STENCIL = {'nearest': 1, 'linear': 2, 'quadratic': 3}
EPS = {'f32': float(np.finfo(np.float32).eps), 'f64': float(np.finfo(np.float64).eps)}
NPDT = {'f32': np.float32, 'f64': np.float64}
LC_THREADS, LC_RSTRIP = 256, 4        # csrc/lcone.hip: lanes of a work-group, radii of a lane's strip (NR crosses it)


def cubes():
    """(NSIM,) + EXT float64, seeded"""
    return np.random.default_rng(20261020).normal(size=(NSIM,) + EXT)


def roll3(roll):
    return (0, 0, 0) if roll is None else (roll,) * 3 if isinstance(roll, int) else tuple(roll)


def unit_vectors(angs):
    theta, phi = np.asarray(angs, dtype=np.float64)
    st = np.sin(theta)
    return np.stack([st * np.cos(phi), st * np.sin(phi), np.cos(theta)])


def fixture_angs():
    """(2, 230): the 192 pixel centres of nside 4, both poles (exact zeros: x = y = 0, z = dc / sim_res, an integer at the
    node radius), the four equatorial axis directions, 32 seeded random directions"""
    from bayeslim_amd import healpix
    th, ph = healpix.pix2ang(4)
    rng = np.random.default_rng(7)
    rt, rp = np.arccos(rng.uniform(-1, 1, 32)), rng.uniform(0, 2 * np.pi, 32)
    theta = np.concatenate([th, [0.0, np.pi], [np.pi / 2] * 4, rt])
    phi = np.concatenate([ph, [0.0, 0.0], np.arange(4) * np.pi / 2, rp])
    return np.stack([theta, phi])


def _landing(k, r):
    """a float64 v with (v * r) / SIM_RES an integer exactly: the first of k, k + 1, ... (k - 1, ... for a negative k) that
    a float64 near k SIM_RES / r lands on (not every integer has one: a step of v can step over it)"""
    for j in range(200):
        kk = k + j if k > 0 else k - j
        v0 = kk * SIM_RES / r
        for v in (v0, np.nextafter(v0, np.inf), np.nextafter(v0, -np.inf)):
            if (v * r) / SIM_RES == kk:
                return v
    raise AssertionError('no float64 lands on an integer near %r at r = %r' % (k, r))


def special_vectors():
    """(3, 30) directions handed to the kernel as they are: the six axis directions (exact zeros, and at the node radius
    8996 the integer coordinate +-4498), and for every radius of R two directions with a coordinate exactly on an integer
    (positive on x, negative on y) and two whose z lands in the last voxel of the z axis (from above zero and from below:
    floor(z) mod Nz = Nz - 1, so the upper z corner wraps to 0)"""
    v = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    for r in R:
        v.append([_landing(37, r), 0.3, 0.4])
        v.append([0.25, _landing(-1201, r), -0.6])
        v.append([0.5, -0.1, (EXT[2] * 600 - 0.25) * SIM_RES / r])
        v.append([-0.7, 0.2, -0.25 * SIM_RES / r])
    return np.asarray(v, dtype=np.float64).T.copy()


def random_vectors(n=257):
    v = np.random.default_rng(11).normal(size=(3, n))
    return v / np.sqrt((v ** 2).sum(axis=0))


def kernel_vectors():
    """(3, 485): nside-4 pixel centres, the special directions and the random set"""
    from bayeslim_amd import healpix
    return np.concatenate([unit_vectors(np.stack(healpix.pix2ang(4))), special_vectors(), random_vectors()], axis=1)


# the fixture: name -> (order of sim_r, rinterp, interp, roll, angs given)
def fixture_cases(pinned=True):
    cases = {}
    rolls = {'asc': ROLLS, 'desc': [None, (-9, 13, 7)]}
    for order in ('asc', 'desc'):
        for ri in ('nearest', 'linear'):
            for si in INTERP:
                for k, roll in enumerate(rolls[order]):
                    cases['%s_%s_%s_roll%d' % (order, ri, si, k)] = (order, ri, si, roll, True)
    for ri in ('nearest', 'linear'):
        for si in INTERP:
            for k, roll in enumerate([None, (1, 0, -2)]):
                cases['plane_%s_%s_roll%d' % (ri, si, k)] = ('asc', ri, si, roll, False)
    for si in INTERP:                                                      # cube2map itself: cube 1 at R[2]
        cases['map_%s' % si] = ('map', 'nearest', si, 3, True)
        cases['map_plane_%s' % si] = ('map', 'nearest', si, (1, 0, -2), False)
    if not pinned:
        cases = {'info_quadratic_%s' % si: ('asc', 'quadratic', si, None, True) for si in INTERP}
    return cases


def golden():
    """lcone.npz as a dict of numpy arrays, loaded once and never modified by a test"""
    if GOLDEN not in _CACHE:
        with np.load(GOLDEN) as f:
            _CACHE[GOLDEN] = {k: f[k] for k in f.files}
    return _CACHE[GOLDEN]


# ------------------------------------------------------------------------------------------ restatement of the kernel
def stencil(sim_r, r, rinterp):
    """(cube_idx (Nr, 3), weight (Nr, 3), S): the S cubes nearest to every r (ties: the lower index) in index order;
    weights 1 / (1 - t, t) / Lagrange through the three"""
    S = STENCIL[rinterp]
    sim_r, r = np.asarray(sim_r, dtype=np.float64), np.atleast_1d(np.asarray(r, dtype=np.float64))
    idx, wgt = np.zeros((len(r), 3), dtype=np.int32), np.zeros((len(r), 3))
    for i, ri in enumerate(r):
        near = sorted(sorted(range(len(sim_r)), key=lambda j: (abs(ri - sim_r[j]), j))[:S])
        x = sim_r[near]
        idx[i, :S] = near
        if S == 1:
            wgt[i, 0] = 1.0
        elif S == 2:
            t = (ri - x[0]) / (x[1] - x[0])
            wgt[i, :2] = 1.0 - t, t
        else:
            for a in range(3):
                b, c = [k for k in range(3) if k != a]
                wgt[i, a] = (ri - x[b]) * (ri - x[c]) / ((x[a] - x[b]) * (x[a] - x[c]))
    return idx, wgt, S


def _axis(x, N, roll, linear):
    if not linear:
        i = np.rint(x).astype(np.int64) % N
        return (i - roll) % N, None, None
    fl = np.floor(x)
    i0 = fl.astype(np.int64) % N
    return (i0 - roll) % N, ((i0 + 1) % N - roll) % N, x - fl


def restate(sims, vec, dc, idx, wgt, S, sim_res, roll, interp):
    """float64 restatement of rime_lcone_fwd: sims (Nsim, Nx, Ny, Nz), vec (3, Npix) or None (plane), dc (Nr,), the stencil
    table, roll three ints of any sign -> (Nr, Npix) or (Nr, Nx, Ny)"""
    sims = np.asarray(sims, dtype=np.float64)
    Nx, Ny, Nz = sims.shape[1:]
    rx, ry, rz = roll3(roll)
    lin = interp == 'linear'
    lerp = lambda a, b, f: a * (1.0 - f) + b * f
    out = []
    for i, d in enumerate(np.asarray(dc, dtype=np.float64)):
        if vec is None:
            xs = ((np.arange(Nx) - rx) % Nx)[:, None]
            ys = ((np.arange(Ny) - ry) % Ny)[None, :]
            z0, z1, fz = _axis(np.float64(d) / sim_res, Nz, rz, lin)
        else:
            x0, x1, fx = _axis((vec[0] * d) / sim_res, Nx, rx, lin)
            y0, y1, fy = _axis((vec[1] * d) / sim_res, Ny, ry, lin)
            z0, z1, fz = _axis((vec[2] * d) / sim_res, Nz, rz, lin)
        acc = 0.0
        for s in range(S):
            c = sims[idx[i, s]]
            if vec is None:
                val = lerp(c[xs, ys, z0], c[xs, ys, z1], fz) if lin else c[xs, ys, z0]
            elif not lin:
                val = c[x0, y0, z0]
            else:
                c00, c01 = lerp(c[x0, y0, z0], c[x1, y0, z0], fx), lerp(c[x0, y0, z1], c[x1, y0, z1], fx)
                c10, c11 = lerp(c[x0, y1, z0], c[x1, y1, z0], fx), lerp(c[x0, y1, z1], c[x1, y1, z1], fx)
                val = lerp(lerp(c00, c10, fy), lerp(c01, c11, fy), fz)
            acc = wgt[i, s] * val if s == 0 else acc + wgt[i, s] * val
        out.append(acc)
    return np.asarray(out)


def roundings(interp, S, plane):
    """K: the roundings on the longest path of the kernel's operation order (module docstring)"""
    spatial = 0 if interp == 'nearest' else 4 if plane else 12
    return spatial + 1 + S


def bound(prec, interp, S, plane, wgt, cube_max):
    """(Nr,) |kernel - restatement| allowed per radius: K (eps_T + eps_64) W M"""
    W = np.abs(np.asarray(wgt)[:, :S]).sum(axis=1)
    return roundings(interp, S, plane) * (EPS[prec] + EPS['f64']) * W * cube_max


def restate_fixture(name, pinned=True):
    """the restatement of one fixture case from the recorded inputs"""
    G = golden()
    order, ri, si, roll, sphere = fixture_cases(pinned)[name]
    vec = unit_vectors(G['angs']) if sphere else None
    if order == 'map':
        idx, wgt, S = np.zeros((1, 3), dtype=np.int32), np.array([[1.0, 0.0, 0.0]]), 1
        return restate(G['sims'][1:2], vec, R[2:3], idx, wgt, S, SIM_RES, roll, si)[0]
    idx, wgt, S = stencil(SIM_R[order], R, ri)
    return restate(G['sims'], vec, R, idx, wgt, S, SIM_RES, roll, si)


def rel_err(x, ref):
    ref = np.asarray(ref)
    scale = np.abs(ref).max()
    return np.abs(np.asarray(x) - ref).max() / scale if scale > 0 else np.abs(np.asarray(x) - ref).max()
