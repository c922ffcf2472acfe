"""
Shared by tests/test_redcal_host.py, tests/test_redcal_gpu.py and tests/golden/make_golden_redcal.py: the float64 restatement
of rime_redvis_fwd / rime_redvis_bwd (numpy, explicit loops over the tables, written from the formulas of include/rime_hip.h),
the kernel cases, the derived accuracy bound, and the names of the model cases recorded in tests/golden/redcal.npz.

The bound (derived, not measured; fixed by the design of the kernel, not by its results).  With u = 2^-24 (float32) or
2^-53 (float64), per real component of every element:
  forward   out = fl(vis + sign * model), one rounding (sign * model is exact):   |err| <= u (|vis| + |model|)
  backward  a sum of n members in any order:   |err| <= gamma_n sum |terms|,   gamma_n = n u / (1 - n u),
            n = (members of the group) * (times of the model time)  (Higham, Accuracy and Stability of Numerical Algorithms,
            section 4.2: gamma_(n-1) for n - 1 additions, whatever their order); the final product with sign is exact.
The tests assert error / bound <= 1 for every component and print the worst ratio.  n = 0: bound 0, asserted as equality.
The inputs of the kernel cases lie on the grid 2^-20 with |x| < 8 (23 bits: exact in float32), and no case sums more than
2^10 of them (33 bits), so every sum below is EXACT in float64 in any order: the restatement has no rounding of its own to
account for.  In float32 the kernel's sums need more than 24 bits and do round; in float64 the kernels must reproduce the
restatement.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(HERE, 'golden', 'redcal.npz')) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


# model cases of the fixture: tag -> (class, param_type, keywords of the case)
MODEL_CASES = {
    'rv_com': ('RedVisModel', 'com', {}),
    'rv_undo': ('RedVisModel', 'com', dict(undo=True)),
    'rv_p0': ('RedVisModel', 'com', dict(p0=True)),
    'rv_tsel': ('RedVisModel', 'com', dict(tsel=[0, 2])),
    'rv_amp_phs': ('RedVisModel', 'amp_phs', {}),
    'rv_full': ('RedVisModel', 'com', dict(full=True)),                 # the model's baseline axis is already the input's
    'vm_com': ('VisModel', 'com', {}),
    'vm_undo': ('VisModel', 'com', dict(undo=True)),
    'vm_p0': ('VisModel', 'com', dict(p0=True)),
    'vm_tsel': ('VisModel', 'com', dict(tsel=[0, 2])),
    'vm_bsel': ('VisModel', 'com', dict(bsel=[5, 2, 9, 20, 27])),
    'vm_amp_phs': ('VisModel', 'amp_phs', {}),
}
NT, NF = 3, 5


def csr(index, N):
    """offsets [N + 1] and members (ascending) of a map index -> [0, N), with plain loops"""
    lists = [[] for _ in range(N)]
    for i, r in enumerate(index):
        lists[int(r)].append(i)
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    return np.asarray(off), np.asarray([i for l in lists for i in l], dtype=np.int64)


def fwd_ref(vis, model, red, tmap, sign):
    """out[p, b, t, f] = vis[p, b, t, f] + sign * model[p, red[b], tmap[t], f]; vis [P, Nbl, Nt, Nf] complex128 or None,
    model [P, Nred, Ntm, Nf]; returns (out, |vis| + |model| per real component as a complex array of bounds)"""
    P, Nf = model.shape[0], model.shape[3]
    Nbl, Nt = len(red), (len(tmap) if tmap is not None else model.shape[2])
    out = np.zeros((P, Nbl, Nt, Nf), dtype=np.complex128)
    mag = np.zeros((P, Nbl, Nt, Nf), dtype=np.complex128)
    for p in range(P):
        for b in range(Nbl):
            for t in range(Nt):
                m = model[p, red[b], t if tmap is None else tmap[t]]
                v = vis[p, b, t] if vis is not None else np.zeros(Nf, dtype=np.complex128)
                out[p, b, t] = v + sign * m
                mag[p, b, t] = (np.abs(v.real) + np.abs(m.real)) + 1j * (np.abs(v.imag) + np.abs(m.imag))
    return out, mag


def bwd_ref(gout, goff, gmem, toff, tmem, sign):
    """gmodel[p, r, t', f] = sign * sum over the times of t' and the baselines of r of gout[p, b, t, f]; returns
    (gmodel, sum |terms| per real component, n [Nred, Ntm])"""
    P, Nbl, Nt, Nf = gout.shape
    Nred, Ntm = len(goff) - 1, len(toff) - 1
    gm = np.zeros((P, Nred, Ntm, Nf), dtype=np.complex128)
    mag = np.zeros((P, Nred, Ntm, Nf), dtype=np.complex128)
    n = np.zeros((Nred, Ntm), dtype=np.int64)
    for r in range(Nred):
        for tp in range(Ntm):
            for q in range(toff[tp], toff[tp + 1]):
                for m in range(goff[r], goff[r + 1]):
                    g = gout[:, gmem[m], tmem[q]]
                    gm[:, r, tp] += g
                    mag[:, r, tp] += np.abs(g.real) + 1j * np.abs(g.imag)
                    n[r, tp] += 1
    return sign * gm, mag, n


def gamma(n, u):
    return n * u / (1 - n * u)


def ratio(got, want, bound):
    """worst |got - want| / bound over the real components; a zero bound demands equality (ratio 0 or inf)"""
    worst = 0.0
    for part in ('real', 'imag'):
        e = np.abs(getattr(got, part).astype(np.float64) - getattr(want, part))
        b = getattr(bound, part)
        r = np.where(b > 0, e / np.where(b > 0, b, 1), np.where(e == 0, 0.0, np.inf))
        worst = max(worst, float(r.max()))
    return worst


def fwd_bound(mag, prec):
    return U[prec] * mag


def bwd_bound(mag, n, prec):
    g = gamma(n, U[prec])[None, :, :, None]
    return g * mag.real + 1j * (g * mag.imag)


def hex7_red():
    """the hex-7 grouping of the fixture: (red [28], Nred)"""
    g = golden()
    return g['red'].astype(np.int64), int(g['red'].max()) + 1


def ragged_red():
    """case (b): 304 baselines; groups 1, 2, 4 singletons, group 3 empty, group 0 the other 301 (more than the 4 x 64 members a
    backward block takes per round of its waves, and not a multiple of the 4 waves), spread over the whole list"""
    red = np.zeros(304, dtype=np.int64)
    red[[7, 150, 303]] = [1, 2, 4]
    return red, 5


# kernel cases: name -> dict(red=callable -> (red, Nred), Nt, Ntm, tmap (None: identity), Nf, and the options of the run)
KERNEL_CASES = {
    'a_hex7': dict(red=hex7_red, Nt=3, Ntm=3, tmap=None, Nf=5),
    'b_ragged': dict(red=ragged_red, Nt=3, Ntm=4, tmap=[2, 0, 3], Nf=70),
    'c_single': dict(red=hex7_red, Nt=1, Ntm=1, tmap=None, Nf=1),
    'd_broadcast': dict(red=hex7_red, Nt=3, Ntm=3, tmap=None, Nf=5, broadcast_time=True),
    'e_novis': dict(red=hex7_red, Nt=3, Ntm=3, tmap=None, Nf=5, novis=True),
    'f_minus': dict(red=ragged_red, Nt=3, Ntm=4, tmap=[2, 0, 3], Nf=70, sign=-1),
}


def case_inputs(name, NP, seed=0):
    """(vis | None, model, gout, red, Nred, tmap, sign) of a kernel case in complex128, values on the grid 2^-20 (exact in float32)"""
    c = KERNEL_CASES[name]
    red, Nred = c['red']()
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    P = NP * NP

    def grid(*shape):
        return np.clip(np.round(rng.normal(size=shape) * 2.0 ** 20) / 2.0 ** 20, -7.5, 7.5)

    def rc(*shape):
        return grid(*shape) + 1j * grid(*shape)

    vis = None if c.get('novis') else rc(P, len(red), c['Nt'], c['Nf'])
    model = rc(P, Nred, 1 if c.get('broadcast_time') else c['Ntm'], c['Nf'])
    gout = rc(P, len(red), c['Nt'], c['Nf'])
    return vis, model, gout, red, Nred, c['tmap'], c.get('sign', 1)
