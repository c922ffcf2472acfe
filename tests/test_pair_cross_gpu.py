"""
Pair cross blocks on the GPU (csrc/fringe_xpair.hip through rime_fringe_pair_cross_{fwd,bwd}_block): point-symmetric arrays of
more than 128 antennas against the float64 oracle of the baseline formulation (oracle/rime_oracle.py), at the tolerances the
conjugate-pair form is held to in tests/test_ops_gpu.py (_check_ant_path: visibilities 1e-5, gradients 1e-4 of the maximum).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import rime_oracle as orc
from pair_cross_cases import CROSS_KINDS, EXPECTED, UNCHANGED_KINDS, make_array, make_pairs, seed_of

pytestmark = pytest.mark.gpu

T64 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
TV, TG = 1e-5, 1e-4


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from bayeslim_amd import ops as _ops
    return _ops


def relmax(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def oracle_fringe_sum(psky, blvecs, zenaz, freqs, conj=False):
    """psky (Nt, 1, Npp, Nf, P) float64 / complex128 on the host -> (Npp, Nbl, Nt, Nf), in slices of baselines"""
    out = []
    for t in range(psky.shape[0]):
        rows = []
        for b0 in range(0, len(blvecs), 4096):
            fr = orc.gen_fringe(blvecs[b0:b0 + 4096], zenaz[t, 0], zenaz[t, 1], freqs, conj=conj)     # (nbl, Nf, P)
            rows.append(torch.einsum('bfp,qfp->qbf', fr, psky[t, 0].to(fr.dtype)))
        out.append(torch.cat(rows, dim=1))
    return torch.stack(out, dim=2)


def make_case(ops, kind, full, rng, Nt, Nf, P, cplx=False, Npp=1):
    ant = make_array(kind, rng)
    pairs = make_pairs(len(ant), rng, full)
    blvecs = T64(np.stack([ant[b] - ant[a] for a, b in pairs]))
    freqs = T64(np.linspace(120e6, 180e6, Nf))
    zenaz = T64(np.stack([np.rad2deg(np.arccos(rng.uniform(0, 1, (Nt, P)))), rng.uniform(0, 360, (Nt, P))], axis=1))
    shape = (Nt, 1, Npp, Nf, P)
    psky = rng.normal(size=shape) * np.exp(-9.0 * rng.uniform(size=shape))
    if cplx:
        psky = psky + 1j * rng.normal(size=shape) * np.exp(-9.0 * rng.uniform(size=shape))
    else:
        psky[1, :, :, 2] = np.abs(psky[1, :, :, 2])          # a row without a negative value: the mask-free instantiation
    Ps = ops.pad_to_tile(P)
    sdir = torch.zeros(Nt, 3, Ps, dtype=torch.float64)
    for t in range(Nt):
        sdir[t, :, :P] = orc.pointing_vectors(zenaz[t, 0], zenaz[t, 1])
    return ant, pairs, blvecs, freqs, zenaz, torch.as_tensor(psky), sdir, Ps


def run_both_ways(ops, geom, psky, gv, Ps, cplx):
    """forward and backward through ops.fringe_sum on the matrix-core path"""
    x = torch.zeros(psky.shape[:-1] + (Ps,), dtype=psky.dtype)
    x[..., :psky.shape[-1]] = psky
    x = x.to(torch.complex64 if cplx else torch.float32).cuda().requires_grad_(True)
    prof = []
    ops.PROFILE = prof
    try:
        vis = ops.fringe_sum(x, geom)
        (vis * gv.to(torch.complex64).cuda().conj()).real.sum().backward()
    finally:
        ops.PROFILE = None
    assert [k[0] for k in prof] == ['fringe_ant_fwd_kernel', 'fringe_ant_bwd_kernel']
    return vis.detach(), x.grad[..., :psky.shape[-1]].detach()


def oracle_both_ways(psky, blvecs, zenaz, freqs, conj):
    ref_in = psky.clone().requires_grad_(True)
    ref = oracle_fringe_sum(ref_in, blvecs, zenaz, freqs, conj=conj)
    gv = torch.as_tensor(np.random.default_rng(5).normal(size=tuple(ref.shape))
                         + 1j * np.random.default_rng(6).normal(size=tuple(ref.shape)))
    (ref * gv.conj()).real.sum().backward()
    return ref.detach(), ref_in.grad, gv


def geometry(ops, ant, pairs, blvecs, sdir, freqs, conj=False):
    return ops.FringeGeometry(blvecs.cuda(), sdir.cuda(), freqs, conj=conj, antpos=T64(ant).cuda(), bl_ants=pairs, mfma=True)


@pytest.mark.parametrize('conj', [False, True])
@pytest.mark.parametrize('full', [True, False])
@pytest.mark.parametrize('kind', CROSS_KINDS)
def test_pair_cross_blocks_against_the_oracle(ops, kind, full, conj, monkeypatch):
    """hex-169, hex-217 (two groups), hex-271 (three groups, three cross blocks), a tilted hex-169 (no `flat` licence) and 200
    random antennas (90 pairs + 20 without a partner, z spread, centre away from the origin): the full pair set and a 90 %
    subset with mixed orientations and autocorrelations, both fringe signs, forward and backward, float32, against the float64
    oracle.  The plan: the groups' diagonal blocks on the pair form, the blocks between them on the pair cross form, recorded
    in geom.ant.  With RIME_PAIR_CROSS off: no such key, today's blocks, and a result that agrees to 2e-6 of the maximum without
    being bitwise equal."""
    rng = np.random.default_rng(seed_of(kind, 7))
    Nt, Nf, P = (2, 3, 320) if kind == 'hex271' else (2, 5, 700)
    ant, pairs, blvecs, freqs, zenaz, psky, sdir, Ps = make_case(ops, kind, full, rng, Nt, Nf, P)
    ref, gref, gv = oracle_both_ways(psky, blvecs, zenaz, freqs, conj)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ops, 'PAIR_CROSS', on)
        geom = geometry(ops, ant, pairs, blvecs, sdir, freqs, conj)
        assert geom.ant is not None
        if on:
            diag, cross = EXPECTED[kind]
            assert geom.ant['pair_cross_blocks'] == cross, geom.ant['pair_cross_blocks']
            assert geom.ant['pair_blocks'] == diag, geom.ant['pair_blocks']
            xb = [b for b in geom.ant['blocks_real'] if b.get('xpair')]
            assert len(xb) == len(cross) and all(b['flat'] == int(kind.startswith('hex') and not kind.endswith('t')) for b in xb)
            assert geom.ant['mfma_fwd'] == sum(b['mf_fwd'] for b in geom.ant['blocks_real'])
            assert all(b['mf_fwd'] == 48 and b['mf_bwd_real'] == 6 * 2 * ((b['rows_j'] + 15) // 16) for b in xb)
        else:
            assert 'pair_cross_blocks' not in geom.ant
            assert not any(b.get('xpair') for b in geom.ant.get('blocks_real', geom.ant['blocks']))
        res[on] = run_both_ways(ops, geom, psky, gv, Ps, False)
        ev, eg = relmax(res[on][0], ref), relmax(res[on][1], gref)
        print('%s full=%d conj=%d pair_cross=%d: vis %.2e grad %.2e' % (kind, full, conj, on, ev, eg))
        assert ev < TV and eg < TG
    for a, b in zip(res[True], res[False]):
        assert not torch.equal(a, b)
        assert relmax(a, b) < 2e-6


@pytest.mark.parametrize('kind', UNCHANGED_KINDS)
def test_unchanged_ground_is_bitwise_unchanged(ops, kind, monkeypatch):
    """arrays of at most 128 antennas (the headline's hexagon + outrigger; 60 pairs + 8 singles, which must have no pair block)
    and 150 antennas without symmetry: the same blocks and the same bits with the switch on and off"""
    rng = np.random.default_rng(seed_of(kind, 9))
    ant, pairs, blvecs, freqs, zenaz, psky, sdir, Ps = make_case(ops, kind, False, rng, 2, 4, 500)
    gv = torch.as_tensor(rng.normal(size=(1, len(pairs), 2, 4)) + 1j * rng.normal(size=(1, len(pairs), 2, 4)))
    res, geoms = {}, {}
    for on in (True, False):
        monkeypatch.setattr(ops, 'PAIR_CROSS', on)
        geoms[on] = geometry(ops, ant, pairs, blvecs, sdir, freqs)
        assert 'pair_cross_blocks' not in geoms[on].ant
        res[on] = run_both_ways(ops, geoms[on], psky, gv, Ps, False)
    a, b = geoms[True].ant, geoms[False].ant
    assert set(a) == set(b)
    if kind == 'rand128':
        assert not a.get('pair_blocks')
    for key in a:
        if not key.startswith('blocks'):
            assert torch.equal(a[key], b[key]) if isinstance(a[key], torch.Tensor) else a[key] == b[key], key
            continue
        assert len(a[key]) == len(b[key])
        for x, y in zip(a[key], b[key]):
            assert set(x) == set(y)
            for k in x:
                if isinstance(x[k], torch.Tensor):
                    assert torch.equal(x[k], y[k]), (key, k)
                elif isinstance(x[k], dict):
                    assert all(torch.equal(x[k][q], y[k][q]) if isinstance(x[k][q], torch.Tensor) else x[k][q] == y[k][q] for q in x[k])
                else:
                    assert x[k] == y[k], (key, k)
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


@pytest.mark.parametrize('conj', [False, True])
def test_pair_cross_blocks_complex_psky(ops, conj, monkeypatch):
    """a complex psky with two polarisation products on hex-169: the pair and pair cross blocks take one pass per real plane,
    their slots in the two-pass mask -- against the float64 oracle, both fringe signs"""
    kind = 'hex169'
    rng = np.random.default_rng(seed_of(kind, 11))
    ant, pairs, blvecs, freqs, zenaz, psky, sdir, Ps = make_case(ops, kind, False, rng, 2, 4, 500, cplx=True, Npp=2)
    ref, gref, gv = oracle_both_ways(psky, blvecs, zenaz, freqs, conj)
    geom = geometry(ops, ant, pairs, blvecs, sdir, freqs, conj)
    assert geom.ant['pair_cross_blocks'] == EXPECTED[kind][1]
    assert [bool(b.get('xpair')) for b in geom.ant['blocks_cplx']] == [False, True, False]
    assert float(geom.ant['two_pass_mask_cplx'].sum()) == len(pairs)
    vis, grad = run_both_ways(ops, geom, psky, gv, Ps, True)
    ev, eg = relmax(vis, ref), relmax(grad, gref)
    print('complex psky conj=%d: vis %.2e grad %.2e' % (conj, ev, eg))
    assert ev < TV and eg < TG


def test_pair_cross_kernels_are_repeatable_with_many_blocks_in_flight(ops, monkeypatch):
    """98 304 directions on hex-217: several hundred blocks, two or three to a CU, so that blocks stage while others stream
    MFMAs on the same SIMDs -- three forward and three backward runs are bit-identical and agree with the plan without the
    pair cross blocks to 3e-6 of the maximum"""
    from bayeslim_amd import utils
    ant = utils._make_hex(9, D=14.6)[1]
    n, Nt, Nf, P = len(ant), 2, 24, 98304
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    rng = np.random.default_rng(0)
    blvecs = T64(np.stack([ant[b] - ant[a] for a, b in pairs])).cuda()
    freqs = T64(np.linspace(120e6, 180e6, Nf))
    s = rng.normal(size=(Nt, 3, P))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    s[:, 2] = np.abs(s[:, 2])
    sdir = T64(s).cuda()
    g = torch.as_tensor(rng.normal(size=(1, len(pairs), Nt, Nf)) + 1j * rng.normal(size=(1, len(pairs), Nt, Nf))).to(torch.complex64).cuda()
    psky = torch.as_tensor(rng.normal(size=(Nt, 1, 1, Nf, P))).float().cuda()
    out = {}
    for on in (True, False):
        monkeypatch.setattr(ops, 'PAIR_CROSS', on)
        geom = ops.FringeGeometry(blvecs, sdir, freqs, antpos=T64(ant).cuda(), bl_ants=pairs, mfma=True)
        assert ('pair_cross_blocks' in geom.ant) == on
        bwd = [ops.fringe_adjoint(g, geom).clone() for _ in range(3)]
        fwd = [ops.fringe_sum(psky, geom).clone() for _ in range(3)]
        assert all(torch.equal(bwd[0], b) for b in bwd[1:]) and all(torch.equal(fwd[0], v) for v in fwd[1:])
        out[on] = (bwd[0], fwd[0])
    for a, b in zip(out[True], out[False]):
        err = float((a - b).abs().max()) / float(b.abs().max())
        print('on against off: %.2e' % err)
        assert err < 3e-6


def test_pair_cross_entry_points_reject_bad_arguments():
    """-1 on a bad argument, -2 on a short workspace, before anything is launched"""
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)      # non-null dummy; never dereferenced on a rejected call
    big = 1 << 20
    fwd, bwd = lib.rime_fringe_pair_cross_fwd_block, lib.rime_fringe_pair_cross_bwd_block
    tail = (1, 1, 1, 64, 64, 64)
    assert fwd(one, 65, 64, 0, one, one, one, one, None, one, one, *tail, 1, 1, one, big, None) == -1      # rows_i > 64
    assert fwd(one, 64, 0, 0, one, one, one, one, None, one, one, *tail, 1, 1, one, big, None) == -1       # rows_j = 0
    assert fwd(one, 64, 64, 1, one, one, one, one, None, one, one, *tail, 3, 1, one, big, None) == -1      # pixel stride 3
    assert fwd(one, 64, 64, 1, one, one, one, one, None, None, one, *tail, 1, 1, one, big, None) == -1     # no table
    assert fwd(one, 64, 64, 1, one, one, one, one, None, one, one, 1, 1, 1, 100, 64, 64, 1, 1, one, big, None) == -1   # Pstride % 64
    assert fwd(one, 64, 64, 1, one, one, one, one, None, one, one, *tail, 1, 0, one, big, None) == -1      # sign 0
    assert fwd(one, 64, 64, 1, one, one, one, one, None, one, one, *tail, 1, 1, one, 4, None) == -2
    assert fwd(one, 64, 64, 1, one, one, one, one, None, one, one, *tail, 1, 1, None, big, None) == -2
    assert bwd(one, 0, 64, 0, one, one, one, one, one, *tail, 1, 1, 0, one, one, big, None) == -1
    assert bwd(one, 64, 65, 0, one, one, one, one, one, *tail, 1, 1, 0, one, one, big, None) == -1
    assert bwd(one, 64, 64, 0, one, one, one, one, one, *tail, 1, 1, 0, None, one, big, None) == -1        # no gpsky
    assert bwd(one, 64, 64, 0, one, one, one, one, one, *tail, 2, -1, 0, one, one, 0, None) == -2
