"""
Host checks of tests/interp_common.py (no GPU): the float64 restatements against oracle.rime_oracle.interp and against each
other (adjoint identities), and the case tables of tests/test_interp_gpu.py against the branches of csrc/interp.hip they are
there for -- list lengths of the inverse index around the 16-entry sweep, R % 4, rows beyond one pass, time splits, the
specialised / generic widths.  A case that stops reaching its branch fails here, not silently on the GPU.
"""
import numpy as np
import pytest
import torch

import interp_common as ic
from oracle import rime_oracle as orc


def _dot(a, b):
    return float(np.sum(a * np.conj(b)).real)


def _live_weights(w, seed):
    """the builder's weights with its zeros filled in: the oracle has no notion of a skipped node"""
    fill = np.random.default_rng(seed).uniform(0.25, 1.0, w.shape)
    return np.where(w != 0, w, fill)


@pytest.mark.parametrize('Nnn,cplx', [(1, False), (4, True), (8, False), (12, True), (16, False)])
def test_gather_restatement_against_the_oracle_and_its_adjoint(Nnn, cplx):
    rng = np.random.default_rng(Nnn)
    R, Npb, P = 9, 41, 257
    inds, w0, _ = ic.make_stencil(Nnn, Npb, P, Nnn)
    m = rng.normal(size=(R, Npb)) + (1j * rng.normal(size=(R, Npb)) if cplx else 0)
    g = rng.normal(size=(R, P)) + (1j * rng.normal(size=(R, P)) if cplx else 0)
    w = _live_weights(w0, Nnn)
    out, S, n = ic.gather(m, inds, w)
    ref = orc.interp(torch.as_tensor(m), torch.as_tensor(inds), torch.as_tensor(w)).numpy()
    assert np.abs(out - ref).max() <= 1e-13 * np.abs(ref).max()
    assert (n == Nnn).all()
    # with zeros: same as the oracle (finite map: 0 * m = 0), fewer terms; adjoint identity
    out, S, n = ic.gather(m, inds, w0)
    ref = orc.interp(torch.as_tensor(m), torch.as_tensor(inds), torch.as_tensor(w0)).numpy()
    assert np.abs(out - ref).max() <= 1e-13 * np.abs(ref).max()
    assert (n == (w0 != 0).sum(-1)).all() and n.min() < Nnn
    Sr = S.real + S.imag if cplx else S
    assert (np.abs(out) <= Sr * (1 + 1e-12)).all()
    gm, Sg, ng = ic.gather_adjoint(g, inds, w0, Npb)
    assert gm.shape == m.shape and (ng == ic.csr_lengths(inds, w0, Npb)).all()
    lhs, rhs = _dot(out, g), _dot(m, gm)
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), abs(rhs))


def test_restatements_skip_weight_zero_entries_of_non_finite_data():
    inds, w, planted = ic.make_stencil(3, 41, 257, 4, dead_points=1)
    rng = np.random.default_rng(3)
    m, g = rng.normal(size=(5, 41)), rng.normal(size=(5, 257))
    ref, refg = ic.gather(m, inds, w)[0], ic.gather_adjoint(g, inds, w, 41)[0]
    e = np.flatnonzero(w.reshape(-1) == 0)
    inds.reshape(-1)[e[:3]] = planted[0]
    m[:, planted[0]] = [np.nan, np.inf, np.nan, np.inf, np.nan]
    g[:, planted['dead'][0]] = np.nan
    out, S, _ = ic.gather(m, inds, w)
    gm, Sg, _ = ic.gather_adjoint(g, inds, w, 41)
    assert np.array_equal(out, ref) and np.isfinite(S).all()
    assert np.array_equal(gm, refg) and np.isfinite(Sg).all()


@pytest.mark.parametrize('Nnn,R,Nt', [(1, 37, 3), (4, 66, 6), (9, 72, 7), (2, 37, 9)])
def test_psky_restatement_against_the_oracle_and_its_adjoints(Nnn, R, Nt):
    Npb, Npix, Ps = ic.PSKY_NPB, ic.PSKY_NPIX, ic.PSKY_PS
    rng = np.random.default_rng(10 * Nnn + Nt)
    cut, pos = ic.make_cut(Nt, Nt, Ps, Npix)
    inds, w0, _ = ic.make_stencil(Nnn, Npb, Nt * Ps, Nnn)
    bmap, sky, g = rng.normal(size=(R, Npb)), rng.normal(size=(R, Npix)), rng.normal(size=(R, Nt * Ps))
    w = _live_weights(w0, Nnn)
    psky, S, n = ic.beam_sky(bmap, sky, inds, w, cut)
    sky_ext = torch.cat([torch.as_tensor(sky), torch.zeros(R, 1, dtype=torch.float64)], dim=1)
    ref = (orc.interp(torch.as_tensor(bmap), torch.as_tensor(inds), torch.as_tensor(w)) * sky_ext[:, torch.as_tensor(cut)]).numpy()
    assert np.abs(psky - ref).max() <= 1e-13 * np.abs(ref).max()
    assert (psky[:, cut == Npix] == 0).all() and (n == Nnn + 1).all()
    psky, S, n = ic.beam_sky(bmap, sky, inds, w0, cut)
    gb, Sb, nb = ic.beam_sky_grad_map(g, sky, inds, w0, cut, Npb)
    gs, Ss, ns = ic.beam_sky_grad_sky(g, bmap, inds, w0, cut, Npix)
    # psky is bilinear: <psky, g> = <bmap, grad_map> = <sky, grad_sky>
    lhs = _dot(psky, g)
    assert abs(lhs - _dot(bmap, gb)) <= 1e-13 * abs(lhs) and abs(lhs - _dot(sky, gs)) <= 1e-13 * abs(lhs)
    vis = (pos >= 0).sum(0)
    assert (ns == vis * (Nnn + 1)).all() and (gs[:, vis == 0] == 0).all() and (Ss[:, vis == 0] == 0).all()


# --------------------------------------------------------------------------------------------- builders
def _planted_ok(inds, w, Npb, planted, long=100):
    L = ic.csr_lengths(inds, w, Npb)
    for want in ic.PLANTED[:-1] + (long,):
        assert L[planted[want]] == want
    assert L.min() == 0 and L.max() >= 100 and (L > ic.SWEEP).any()
    share = (w == 0).mean()
    assert (w == 0).any() and 0.07 < share < 0.14
    # the node of the empty list is pointed at by entries of weight 0 only
    at_empty = inds == planted[0]
    assert (w[at_empty] == 0).all()
    return L


def test_cut_builder_keeps_its_promises():
    Ps, Npix = ic.PSKY_PS, ic.PSKY_NPIX
    for Nt in (1, 2) + ic.PSKY_NT:
        cut, pos = ic.make_cut(Nt, Nt, Ps, Npix)
        c2 = cut.reshape(Nt, Ps)
        n = (c2 < Npix).sum(1)
        assert n[-1] == Ps and (Nt == 1 or (n[:-1] < Ps).all())                  # ragged with padding, the last one full
        for t in range(Nt):
            assert (c2[t, :n[t]] < Npix).all() and (c2[t, n[t]:] == Npix).all() and (np.diff(c2[t, :n[t]]) > 0).all()
            assert (pos[t, c2[t, :n[t]]] == np.arange(n[t])).all() and (pos[t] >= 0).sum() == n[t]
        vis = (pos >= 0).sum(0)
        assert vis[ic.NEVER] == 0 and vis[Npix - 1] == 0 and vis[ic.ONCE] == 1 and vis[ic.ALWAYS] == Nt
        if Nt > 2:
            assert c2[1, :n[1]].min() >= (Npix - 1) // 64 * 64                   # step 1: the last 64-pixel tile alone


# --------------------------------------------------------------------------------------------- case tables
def test_gather_table_reaches_every_width_with_both_types_and_partial_blocks():
    assert set(c[0] for c in ic.GATHER_CASES) == set(ic.GATHER_NNN) == {1, 2, 3, 4, 6, 8, 9, 12, 16}
    assert set(ic.GATHER_NNN) - set(ic.GATHER_WIDTHS) == {2, 3, 8, 12}           # interp_gather_kernel<T, NC, 0>
    assert set(ic.GATHER_WIDTHS) <= set(ic.GATHER_NNN)
    assert set(c[3] for c in ic.GATHER_CASES) == {1, 7, 8, 9, 17} and set(c[4] for c in ic.GATHER_CASES) == {1, 255, 256, 257}
    for Nnn in ic.GATHER_NNN:
        mine = [c for c in ic.GATHER_CASES if c[0] == Nnn]
        assert {c[1] for c in mine} == {False, True} and {c[2] for c in mine} == {'f32', 'f64'}
        assert any(c[3] % ic.RT for c in mine) and any(c[4] % 256 for c in mine)
        assert {c[5] for c in mine} == {False, True}
        assert any(c[3] > ic.RT for c in mine) or any(c[4] > 256 for c in mine)
    unplanted = 0
    for Nnn, cplx, prec, R, P, padded in ic.GATHER_CASES:
        inds, w, planted = ic.make_stencil(ic.stencil_seed(1, Nnn, R, P), ic.GATHER_NPB, P, Nnn)
        assert (w == 0).any() and (w != 0).any() and inds.min() >= 0 and inds.max() < ic.GATHER_NPB
        if 0 in planted:
            _planted_ok(inds, w, ic.GATHER_NPB, planted)
        else:
            assert P == 1                                                        # one point cannot hold the lists
            unplanted += 1
    assert unplanted == sum(c[4] == 1 for c in ic.GATHER_CASES)


def test_poison_table():
    assert set(ic.POISON_NNN) == {1, 4, 8, 12}
    assert {n for n in ic.POISON_NNN if n in ic.GATHER_WIDTHS} == {1, 4} and {n for n in ic.POISON_NNN if n not in ic.GATHER_WIDTHS} == {8, 12}
    for Nnn, cplx, prec in ic.POISON_CASES:
        inds, w, planted = ic.make_stencil(ic.stencil_seed(2, Nnn), ic.GATHER_NPB, ic.POISON_P, Nnn, dead_points=2)
        _planted_ok(inds, w, ic.GATHER_NPB, planted)
        assert len(planted['dead']) == 2 and (w[planted['dead']] == 0).all()
    for Nnn in (1, 4):
        inds, w, planted = ic.make_stencil(ic.stencil_seed(2, Nnn), ic.GATHER_NPB, ic.POISON_P, Nnn, all_zero=True)
        assert (w == 0).all() and ic.csr_lengths(inds, w, ic.GATHER_NPB).sum() == 0


def test_scatter_table_reaches_both_row_paths_both_index_paths_and_two_passes():
    RN = sorted({R * (2 if cplx else 1) for R, cplx in ic.SCATTER_ROWS})
    assert RN == [4, 6, 64, 68, 1028, 1030]
    assert [r % 4 == 0 for r in RN] == [True, False, True, True, True, False]   # 16-byte rows / element rows
    assert 68 % ic.ROW_TILE and 68 > ic.ROW_TILE                                 # a partial 64-row tile behind a whole one
    for r in (1028, 1030):                                                       # two passes of the row loop, ragged tails
        assert ic.SCATTER_GRID_ROWS < r < 2 * ic.SCATTER_GRID_ROWS and r % ic.ROW_TILE
    pow2 = {Nnn for Nnn in ic.SCATTER_NNN if Nnn & (Nnn - 1) == 0}
    assert pow2 == {4, 16} and set(ic.SCATTER_NNN) - pow2 == {6, 9}              # shift / divide
    assert {(c[0], c[1] * (2 if c[2] else 1)) for c in ic.SCATTER_CASES} == {(n, r) for n in ic.SCATTER_NNN for r in RN}
    for Nnn in ic.SCATTER_NNN:
        inds, w, planted = ic.make_stencil(ic.stencil_seed(3, Nnn), ic.SCATTER_NPB, ic.SCATTER_P, Nnn)
        L = _planted_ok(inds, w, ic.SCATTER_NPB, planted)
        # around the period of the pipelined walk: none, one slot, one short of a sweep, a sweep, one more, two sweeps + 1
        assert {0, 1, 15, 16, 17, 33} <= set(L.tolist()) and L.sum() == (w != 0).sum()


def test_rows_table():
    assert {c[0] for c in ic.ROWS_CASES} == {1, 7, 8, 9, 23} and {c[3] for c in ic.ROWS_CASES} == {255, 256, 257}
    assert any(c[0] % ic.RB for c in ic.ROWS_CASES) and any(c[0] > 2 * ic.RB for c in ic.ROWS_CASES)
    for cplx in (False, True):                                                   # EW = 1, 2 with gout_stride = P and > P
        assert {c[4] for c in ic.ROWS_CASES if c[1] == cplx} == {0, 37}
        assert {c[2] for c in ic.ROWS_CASES if c[1] == cplx} == {'f32', 'f64'}
    for R, cplx, prec, Npb, extra in ic.ROWS_CASES:
        inds, w, planted = ic.make_stencil(ic.stencil_seed(4, R, Npb), Npb, ic.ROWS_P, 1)
        L = _planted_ok(inds, w, Npb, planted)
        assert (L == 0).sum() > 1 and (L == 1).any() and L.max() >= 100          # selected 0, 1 and many times


def test_big_row_case_needs_a_second_launch_of_both_kernels():
    assert ic.BIG_R == 65535 * 8 + 9
    assert ic.BIG_R > ic.GRID_Y * ic.RT and ic.BIG_R > ic.GRID_Y * ic.RB
    assert (ic.BIG_R - ic.GRID_Y * ic.RT) % ic.RT                                # ... with a partial last block
    assert 2 * ic.BIG_R * (ic.BIG_NPB + 2 * ic.BIG_P) * 4 < 64 << 20             # complex64: map + output + cotangent


def test_psky_table_reaches_every_instantiation_path_and_split():
    assert set(ic.PSKY_NNN) == {1, 2, 4, 8, 9, 16} and set(ic.PSKY_WIDTHS) <= set(ic.PSKY_NNN)
    assert set(ic.PSKY_NNN) - set(ic.PSKY_WIDTHS) == {2, 8}                      # the generic width
    assert [(R % 4 == 0, R > ic.ROW_TILE, R % ic.ROW_TILE != 0) for R in ic.PSKY_R] == \
        [(False, False, True), (False, True, True), (True, True, True)]
    assert {3, 6, 9} <= set(ic.PSKY_NT)
    split = {}
    for R in ic.PSKY_R:
        for Nt in ic.PSKY_NT:
            S, Tc = ic.sky_grad_splits(R, ic.PSKY_NPIX, Nt)
            split[Nt] = (S, Tc, Nt - (S - 1) * Tc)
            assert split[Nt] == ic.sky_grad_splits(ic.PSKY_R[0], ic.PSKY_NPIX, Nt) + (Nt - (S - 1) * Tc,)
    # no split; whole splits of 3 steps; a ragged last split
    assert split[3] == (1, 3, 3) and split[6] == (2, 3, 3) and split[9] == (3, 3, 3) and split[7] == (2, 4, 3)
    assert set(ic.PSKY_CASES) == {(n, p, R, Nt) for n in ic.PSKY_NNN for p in ('f32', 'f64') for R in ic.PSKY_R for Nt in ic.PSKY_NT}
    for Nnn in ic.PSKY_NNN:
        for Nt in ic.PSKY_NT:
            inds, w, planted = ic.make_stencil(ic.stencil_seed(6, Nnn, Nt), ic.PSKY_NPB, Nt * ic.PSKY_PS, Nnn)
            _planted_ok(inds, w, ic.PSKY_NPB, planted)
