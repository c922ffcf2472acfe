"""
Progressions in the conjugate-pair form (round 6; DESIGN.md 5.1, csrc/fringe_mfma.hip "PROGRESSIONS"): the host orders the rows
of a pair block so that octets hold two 4-term arithmetic progressions of ONE step, and the pair backward kernel evaluates
one phasor of such a quad and rotates it to the other three.  No GPU needed: the row order, the octet mask (the kernel's
test, restated in ops._pair_ap_mask), the slot tables, and a float32 model of the rotation chain against float64 phasors.
"""
import numpy as np
import pytest
import torch

from bayeslim_amd import ops, utils

C_LIGHT = 2.99792458e8
SIDES = {'hex127+1': 7, 'hex37': 4, 'hex61': 5}


def _hex(kind):
    v = utils._make_hex(SIDES[kind], D=14.6)[1]
    if kind.endswith('+1'):
        v = np.vstack([v, [[250.0, 0.0, 0.0]]])                   # the benchmark's hera128 geometry
    return v


def _layout(P, ap):
    return ops._pair_layout(P, ap=ap) if len(P) > 64 else ops._pair_layout(P, rows=32, hub_ok=False, ap=ap)


def _mask_1nm(pos):
    """the kernel's test in plain numpy: step = row 1 - row 0; bit m: rows 8m..8m+3 and 8m+4..8m+7 are r + k step within 1 nm"""
    step, mask = pos[1] - pos[0], 0
    for m in range(len(pos) // 8):
        ok = True
        for q in (8 * m, 8 * m + 4):
            for k in (1, 2, 3):
                ok = ok and bool((np.abs(pos[q + k] - pos[q] - k * step) <= 1e-9).all())
        mask |= int(ok) << m
    return mask


def _plain_block(P, rng, full):
    """the 128 x 128 slot tables of a diagonal block as _antenna_blocks builds them: direct[i, j] = b for baseline b from
    antenna i to j, or conj[i, j] = b for one from j to i"""
    n = len(P)
    direct = np.full((128, 128), -1, dtype=np.int32)
    conj = np.full((128, 128), -1, dtype=np.int32)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if full or rng.random() < 0.9]
    for b, k in enumerate(rng.permutation(len(pairs))):
        i, j = pairs[k]
        if full or rng.random() < 0.5:
            direct[i, j] = b
        else:
            conj[i, j] = b
    return dict(nrows=n, cross=0, direct=torch.as_tensor(direct.reshape(-1)), conj=torch.as_tensor(conj.reshape(-1))), len(pairs)


@pytest.mark.parametrize('kind,min_octets', [('hex127+1', 6), ('hex37', 1), ('hex61', 2)])
def test_row_order_exposes_progressions(kind, min_octets):
    """hex-127 + outrigger (the headline array), hex-37 (32-row form) and hex-61: the new rows are a permutation of the plain
    rows (same antennas, same partners, same hub), at least `min_octets` octets qualify under the kernel's 1 nm test, the
    qualifying octets come first and all their quads run along the same step"""
    P = _hex(kind)
    f0, p0, hub0, c0 = _layout(P, False)
    f1, p1, hub1, c1 = _layout(P, True)
    assert hub0 == hub1 and np.array_equal(c0, c1)
    assert sorted(zip(f0, p0)) == sorted(zip(f1, p1)) and len(set(f1)) == len(f1)
    pos = P[f1] - c1
    mask = _mask_1nm(pos)
    assert mask == ops._pair_ap_mask(pos)
    noct = bin(mask).count('1')
    assert noct >= min_octets and mask == (1 << noct) - 1, bin(mask)
    assert noct >= bin(_mask_1nm(P[f0] - c0)).count('1')
    step = pos[1] - pos[0]
    for q in range(0, 8 * noct, 4):
        assert np.abs(pos[q + 1:q + 4] - pos[q:q + 3] - step).max() <= 1e-9


@pytest.mark.parametrize('kind', ['hex127+1', 'hex37', 'hex61'])
@pytest.mark.parametrize('full', [True, False])
def test_pair_block_slots_exactly_once(kind, full, monkeypatch):
    """every baseline slot of the plain block appears exactly once across direct, conj and centre of the pair block -- in the
    forward's tables (the plain order, whatever RIME_PAIR_AP says) and in the backward's own (blk['bwd'], the progression
    order) -- and joins the same two antennas in both"""
    P = _hex(kind)
    blk, nbl = _plain_block(P, np.random.default_rng(3), full)
    ends = {}
    for on in (False, True):
        monkeypatch.setattr(ops, 'PAIR_AP', on)
        pb = ops._pair_block(blk, P, torch.device('cpu'))
        assert pb is not None and pb['pair'] == 1 and pb['flat'] == 1
        assert (pb['centre'] is not None) == (kind == 'hex127+1')
        assert on or pb['bwd'] is None
        fwd_firsts = pb['firsts']
        hub = pb['hub']
        if on and pb['bwd'] is not None:
            pb = pb['bwd']
            assert ops._pair_ap_mask(pb['pos'].numpy()) != 0
        tabs = [pb['direct'].numpy(), pb['conj'].numpy()] + ([pb['centre'].numpy()] if pb['centre'] is not None else [])
        slots = np.concatenate([t[t >= 0] for t in tabs])
        assert len(slots) == nbl and np.array_equal(np.sort(slots), np.arange(nbl))
        vrow = {}
        for k, (a, b) in enumerate(zip(pb['firsts'], pb['partner'])):
            vrow[k] = a
            if b >= 0:
                vrow[64 + k] = b
        d = pb['direct'].numpy().reshape(128, 128)
        cj = pb['conj'].numpy().reshape(128, 128)
        e = {int(d[i, j]): (vrow[i], vrow[j]) for i, j in zip(*np.nonzero(d >= 0))}
        e.update({int(cj[i, j]): (vrow[j], vrow[i]) for i, j in zip(*np.nonzero(cj >= 0))})
        if pb['centre'] is not None:
            ce = pb['centre'].numpy().reshape(2, 128)
            e.update({int(ce[0, r]): (hub, vrow[r]) for r in np.nonzero(ce[0] >= 0)[0]})
            e.update({int(ce[1, r]): (vrow[r], hub) for r in np.nonzero(ce[1] >= 0)[0]})
        assert len(e) == nbl
        ends[on] = (e, pb['firsts'], fwd_firsts)
    assert ends[True][0] == ends[False][0]
    assert ends[True][2] == ends[False][2]                       # the forward's rows do not depend on the switch
    if kind == 'hex127+1':
        assert ends[True][1] != ends[False][1]


def test_random_symmetric_array_keeps_its_order():
    """a seeded random point-symmetric array (45 pairs + 10 singles): no lattice lines -- the row order is the plain one and
    no octet qualifies, so the kernel runs round 5's code"""
    rng = np.random.default_rng(11)
    h = rng.normal(0, 70.0, (45, 3)) * [1, 1, 0.05]
    P = np.vstack([h, -h, rng.normal(0, 70.0, (10, 3)) * [1, 1, 0.05]])
    P = P[rng.permutation(len(P))] + [31.7, -12.3, 4.1]
    f0, p0, hub0, c0 = _layout(P, False)
    f1, p1, hub1, c1 = _layout(P, True)
    assert (f0, p0, hub0) == (f1, p1, hub1)
    assert ops._pair_ap_mask(P[f1] - c1) == 0 and _mask_1nm(P[f1] - c1) == 0


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _rot(c, s, dc, ds):
    """the kernel's rotation in float32: a product, then one fused multiply-add (emulated in float64: the exact product of two
    float32 values plus a float32 value, rounded once more -- the double rounding is negligible against what is measured)"""
    c64, s64 = c.astype(np.float64), s.astype(np.float64)
    t = _f32(c64 * dc)
    w = _f32(s64 * dc)
    return _f32(-s64 * ds + t), _f32(c64 * ds + w)


def chain_error_model(npix=200000, seed=0):
    """float32 model of the chain E1 (evaluated), E0 = E1 conj(D), E2 = E1 D, E3 = E2 D against float64 phasors on the
    headline geometry: directions of the visible hemisphere, 120..180 MHz, the hex-127 step (14.6 m along x), quads anywhere
    on the array (|r| up to 90 m).  Returns arrays of |E - E_exact| (radians, |E| = 1): 'parent' = a phasor evaluated as all
    are today (float32 fraction of the float64 phase, float32 sine / cosine), 'rot1' one rotation away, 'rot2' two."""
    rng = np.random.default_rng(seed)
    s = rng.normal(size=(npix, 3))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    s[:, 2] = np.abs(s[:, 2])
    nu = rng.uniform(120e6, 180e6, npix) / C_LIGHT
    r0 = np.stack([rng.uniform(-90, 50, npix), rng.uniform(-90, 90, npix), np.zeros(npix)], axis=1)
    d = np.array([14.6, 0.0, 0.0])

    def exact(r):
        return np.exp(2j * np.pi * nu * (r * s).sum(1))

    def evaluated(r):
        ph = nu * (r * s).sum(1)
        ang = 2 * np.pi * _f32(ph - np.floor(ph)).astype(np.float64)
        return _f32(np.cos(ang)), _f32(np.sin(ang))

    def err(c, sn, r):
        return np.abs(c.astype(np.float64) + 1j * sn.astype(np.float64) - exact(r))

    dc, ds = evaluated(np.broadcast_to(d, r0.shape))
    c1, s1 = evaluated(r0 + d)
    c0, s0 = _rot(c1, s1, dc, -ds)
    c2, s2 = _rot(c1, s1, dc, ds)
    c3, s3 = _rot(c2, s2, dc, ds)
    return {'parent': np.concatenate([err(*evaluated(r0 + k * d), r0 + k * d) for k in range(4)]),
            'rot1': np.concatenate([err(c0, s0, r0), err(c2, s2, r0 + 2 * d)]),
            'rot2': err(c3, s3, r0 + 3 * d)}


def test_rotation_chain_error_budget():
    """the model behind profiles/r06/pair_bwd_ap.txt.  An evaluated phasor is off by the float32 rounding of its phase fraction
    (<= 2 pi 2^-25 rad) and of its sine and cosine (<= 2^-25 each): 2.3e-7 at worst.  A rotated one adds the error of D once
    or twice and, per rotation, two float32 roundings per component (<= 2^-25 each).  Bounds from those formats, not from
    the kernel: one rotation <= 2 evaluations + 0.9e-7 < 3 x, two <= 3 evaluations + 1.7e-7 < 4.5 x the worst evaluated
    phasor -- 1e-6, two decades inside the 1e-4 gradient contract (a gradient entry sums products of two phasors with
    visibility gradients: its relative error is of the order of twice the phasor error)."""
    err = chain_error_model()
    worst_eval = 2 * np.pi * 2.0 ** -25 + np.sqrt(2) * 2.0 ** -25
    print('phasor error [rad]  max / p99 / rms:')
    for k in ('parent', 'rot1', 'rot2'):
        print('  %-6s %.2e  %.2e  %.2e' % (k, err[k].max(), np.quantile(err[k], 0.99), np.sqrt((err[k] ** 2).mean())))
    assert err['parent'].max() <= worst_eval * 1.01
    assert err['rot1'].max() <= 3.0 * worst_eval
    assert err['rot2'].max() <= 4.5 * worst_eval
    assert err['rot2'].max() < 1e-4 / 50
