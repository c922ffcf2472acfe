"""
Host-side checks of the pair cross plan (ops._pair_cross_plan: numpy in, numpy out, no device): symmetric groups of a
point-symmetric array with more than 128 antennas, the slot tables of the blocks between them, the arrays that must decline,
and the build's scan record of the new kernels.
"""
import os
import re

import numpy as np
import pytest

import kernel_asm
from pair_cross_cases import CROSS_KINDS, EXPECTED, UNCHANGED_KINDS, make_array, make_pairs, seed_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('full', [True, False])
@pytest.mark.parametrize('kind', CROSS_KINDS)
def test_plan_groups_and_tables(kind, full):
    """every group is a set of rows with their mirrors about ONE centre, no group exceeds 64 rows, and every baseline between
    two groups sits in exactly one entry of exactly one block's tables (the baselines inside a group belong to its diagonal
    block); the `flat` licence exactly where the array is coplanar"""
    from bayeslim_amd import ops
    rng = np.random.default_rng(seed_of(kind))
    ant = make_array(kind, rng)
    pairs = make_pairs(len(ant), rng, full)
    plan = ops._pair_cross_plan(ant, pairs)
    assert plan is not None
    c = plan['centre']
    group_of = {}
    for g, grp in enumerate(plan['groups']):
        assert 0 < len(grp['firsts']) <= ops.PAIR_ROWS == 64 and len(grp['firsts']) == len(grp['partner'])
        for a, b in zip(grp['firsts'], grp['partner']):
            assert a not in group_of and b not in group_of
            group_of[a] = g
            if b >= 0:
                group_of[b] = g
                assert np.abs(ant[a] + ant[b] - 2 * c).max() <= 1e-9
        assert sorted(plan['ants'][g]) == sorted(a for a, h in group_of.items() if h == g)
    assert sorted(group_of) == list(range(len(ant)))
    assert [len(g['firsts']) for g in plan['groups']] == [r for _, r, _ in EXPECTED[kind][0]]
    assert [(plan['cross'][k]['rows_i'], plan['cross'][k]['rows_j']) for k in sorted(plan['cross'])] == EXPECTED[kind][1]
    seen = {}
    for (gi, gj), blk in plan['cross'].items():
        assert gi < gj
        fi, pi = plan['groups'][gi]['firsts'], plan['groups'][gi]['partner']
        fj, pj = plan['groups'][gj]['firsts'], plan['groups'][gj]['partner']
        assert (blk['rows_i'], blk['rows_j']) == (len(fi), len(fj)) and blk['pos'].shape == (len(fi) + len(fj), 3)
        assert np.abs(blk['pos'] - (ant[fi + fj] - c)).max() <= 1e-9
        assert blk['flat'] == int(kind.startswith('hex') and not kind.endswith('t'))
        if blk['flat']:
            assert (blk['pos'][:, 2] == 0).all()
        row_ant = {k: a for k, a in enumerate(fi)}
        row_ant.update({64 + k: b for k, b in enumerate(pi) if b >= 0})
        col_ant = {k: a for k, a in enumerate(fj)}
        col_ant.update({64 + k: b for k, b in enumerate(pj) if b >= 0})
        for name in ('direct', 'conj'):
            tab = blk[name]
            assert tab.shape == (128, 128) and tab.dtype == np.int32
            for r, q in zip(*np.nonzero(tab >= 0)):
                slot = int(tab[r, q])
                assert slot not in seen
                seen[slot] = (gi, gj)
                a1, a2 = (row_ant[r], col_ant[q]) if name == 'direct' else (col_ant[q], row_ant[r])
                assert pairs[slot] == (a1, a2)
    between = [s for s, (a, b) in enumerate(pairs) if group_of[a] != group_of[b]]
    assert sorted(seen) == between


@pytest.mark.parametrize('kind', CROSS_KINDS)
def test_plan_tables_reproduce_the_visibilities(kind):
    """the algebra the kernels run, in float64 on the host: Pcc, Pss, Pcs, Psc of the rows' phasors, sent through the block's
    tables as the forward does, give sum_p w conj(E_a) E_b for every baseline between two groups; and the four N planes of the
    backward built from a gradient through the same tables give the gradient of that sum"""
    from bayeslim_amd import ops
    rng = np.random.default_rng(seed_of(kind, 3))
    ant = make_array(kind, rng)
    pairs = make_pairs(len(ant), rng, False)
    plan = ops._pair_cross_plan(ant, pairs)
    npix = 40
    s = rng.normal(size=(3, npix))
    s /= np.linalg.norm(s, axis=0)
    w = rng.normal(size=npix)
    k = 150e6 / 2.99792458e8
    E = np.exp(2j * np.pi * k * (ant @ s))                                   # (Nant, npix)
    ref = np.array([(w * np.conj(E[a]) * E[b]).sum() for a, b in pairs])
    g = rng.normal(size=len(pairs)) + 1j * rng.normal(size=len(pairs))
    gref = sum((np.conj(g[n]) * np.conj(E[a]) * E[b]).real for n, (a, b) in enumerate(pairs)
               if any(n in blk['direct'] or n in blk['conj'] for blk in plan['cross'].values()))
    out = np.full(len(pairs), np.nan, dtype=complex)
    gsum = np.zeros(npix)
    for blk in plan['cross'].values():
        ri, rj = blk['rows_i'], blk['rows_j']
        X = np.exp(2j * np.pi * k * (blk['pos'][:ri] @ s))
        Y = np.exp(2j * np.pi * k * (blk['pos'][ri:] @ s))
        Pcc, Pss = (X.real * w) @ Y.real.T, (X.imag * w) @ Y.imag.T
        Pcs, Psc = (X.real * w) @ Y.imag.T, (X.imag * w) @ Y.real.T
        A, B = (Pcc + Pss) + 1j * (Pcs - Psc), (Pcc - Pss) + 1j * (Pcs + Psc)
        V = np.zeros((128, 128), dtype=complex)
        V[:ri, :rj], V[64:64 + ri, 64:64 + rj], V[64:64 + ri, :rj], V[:ri, 64:64 + rj] = A, A.conj(), B, B.conj()
        d, cj = blk['direct'], blk['conj']
        out[d[d >= 0]] = V[d >= 0]
        out[cj[cj >= 0]] = V[cj >= 0].conj()
        G = np.zeros((128, 128), dtype=complex)                              # gradient with respect to V[r, c]
        G[d >= 0] += g[d[d >= 0]]
        G[cj >= 0] += g[cj[cj >= 0]].conj()
        gA, gA1, gB, gB1 = G[:ri, :rj], G[64:64 + ri, 64:64 + rj], G[64:64 + ri, :rj], G[:ri, 64:64 + rj]
        Ncc, Nss = (gA + gA1 + gB + gB1).real, (gA + gA1 - gB - gB1).real
        Ncs, Nsc = (gA - gA1 + gB - gB1).imag, (-gA + gA1 + gB - gB1).imag
        T1, T2 = Ncc @ Y.real + Ncs @ Y.imag, Nsc @ Y.real + Nss @ Y.imag
        gsum += (X.real * T1 + X.imag * T2).sum(0)
    done = ~np.isnan(out)
    assert done.sum() == sum(int((b['direct'] >= 0).sum() + (b['conj'] >= 0).sum()) for b in plan['cross'].values())
    assert np.abs(out[done] - ref[done]).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(gsum - gref).max() <= 1e-9 * np.abs(gref).max()


@pytest.mark.parametrize('kind', UNCHANGED_KINDS)
def test_plan_declines(kind):
    """at most 128 antennas, or no symmetry of the whole set: today's plan"""
    from bayeslim_amd import ops
    rng = np.random.default_rng(seed_of(kind))
    ant = make_array(kind, rng)
    assert ops._pair_cross_plan(ant, make_pairs(len(ant), rng, True)) is None


def test_plan_declines_repeats_and_too_many_singles():
    """a pair listed twice is not representable; an array whose antennas mostly have no partner would contract and generate
    no less than the groups by index do"""
    from bayeslim_amd import ops
    rng = np.random.default_rng(5)
    ant = make_array('hex169', rng)
    pairs = make_pairs(len(ant), rng, True)
    assert ops._pair_cross_plan(ant, pairs) is not None
    assert ops._pair_cross_plan(ant, pairs + [pairs[17]]) is None
    h = rng.normal(0, 90.0, (10, 3))
    lone = np.vstack([h, -h, rng.normal(0, 90.0, (130, 3))])                 # 10 pairs + 130 singles: 140 rows, three groups
    assert ops._pair_cross_plan(lone, make_pairs(len(lone), rng, True)) is None
    ant = make_array('hex217', rng)                                        # the derivation of the issue for hex-217
    assert ops._plain_plan_cost(ant, make_pairs(len(ant), rng, True)) == (100 + 57 + 192, 128 + 89 + 217)
    # two symmetric sets that are groups by index already, no baseline between them: today's plan is the cheaper one
    hexa = make_array('hex127+1', rng)
    inside = [(i, j) for i in range(128) for j in range(i + 1, 128)] + [(i, j) for i in range(128, 165) for j in range(i + 1, 165)]
    assert ops._pair_cross_plan(np.vstack([hexa, 2 * hexa.mean(0) - hexa[:37]]), inside) is None


def test_scan_record_of_the_pair_cross_kernels():
    """the build scans the gfx950 assembly of csrc/fringe_xpair.hip by itself: no packed f32 instruction in the kernels (their
    blocks share a CU, like the pair kernels'), no scratch, and names that the count of the `*fringe_pair_*` record does not see"""
    obj = os.path.join(ROOT, 'bayeslim_amd', 'lib', 'obj')
    rec = open(os.path.join(obj, 'fringe_xpair.scan')).read()
    assert rec.startswith('no packed-f32 reader') and 'within 24 wait states' in rec, rec
    m = re.search(r'no packed f32 instruction in the (\d+) kernels named \*fringe_xpair_\*', rec)
    assert m and int(m.group(1)) == 6, rec
    assert os.path.getmtime(os.path.join(obj, 'fringe_xpair.scan')) >= os.path.getmtime(os.path.join(obj, 'fringe_xpair.o'))
    asm, kernels, sizes = kernel_asm.read('fringe_xpair')
    assert len(kernels) == 6 and all('fringe_xpair_' in k and 'fringe_pair_' not in k for k in kernels), kernels
    assert not re.findall(r'^\s*scratch_(?:load|store)', asm, flags=re.M)
    assert sizes == [0] * 6
    assert not re.findall(r'^\s*v_pk_(?:add|mul|fma)_f32', asm, flags=re.M)
    src = open(os.path.join(ROOT, 'bayeslim_amd', 'csrc', 'fringe_xpair.hip')).read()
    assert '#if' not in src
