"""
CPU checks of the alm2pix test kit (tests/alm_common.py) and of rime_alm2pix_plan: the case table reaches the branches it
names (MT, padded rows, the long-row predicate, chunk counts and how they are dealt to the splits, from restatements of the
small formulas AND from the library's own plan query, which launches nothing); the numpy emulation of the f16 hi / lo split
stays inside the split part of the derived bound for every case, and the faults the bound is there to catch -- a lost lo
image of either operand, a row scale wrong by a factor of two, a dropped K tail -- all leave the full bound.
"""
import ctypes

import numpy as np
import pytest

import alm_common as ac

ALL = ac.CASES + ac.LONG_CASES
IDS = [ac.case_id(c) for c in ALL]
# From K + C_RED + 48 >= 0.9985 * 2^14 on, the accumulation term (K + c) u32 S alone exceeds the largest lo image there is
# (alm_common: XS); below it a lost lo image must show.  The floor terms of the one-product row are below 2^-24 S.
LO_VISIBLE_K = 16200


def plan(dtype, ys, R, Nc, Npix, direction, packed):
    from bayeslim_amd import _lib
    out = (ctypes.c_int * 6)(*([-7] * 6))
    rc = _lib.lib.rime_alm2pix_plan(dtype, ys, R, Nc, Npix, direction, packed, out)
    return rc, list(out)


# ---------------------------------------------------------------------------------------------- the table and the plan
def test_the_table_holds_the_edges_the_issue_lists():
    rows = {c[0] for c in ac.CASES}
    coef = {c[1] for c in ac.CASES}
    pix = {c[2] for c in ac.CASES}
    assert rows == {1, 32, 33, 64, 65, 128, 129, 200}
    assert coef == {1, 5, 33, 127, 128, 129, 257}
    assert pix == {1, 2, 31, 33, 127, 129, 1110, 1111}
    assert 16 <= len(ac.CASES) <= 32
    assert {ac.mt(c[0]) for c in ac.CASES} == {1, 2, 4}
    assert any(ac.rpad(c[0]) // (ac.mt(c[0]) * 32) > 1 for c in ac.CASES)
    assert len({c[:3] for c in ALL}) == len(ALL)


def test_long_row_cases_sit_on_both_sides_of_the_threshold():
    (b0, b1, b2, b3, f0, f1) = ac.LONG_CASES
    for c in (b0, b1):
        R, Nc, Npix = c[:3]
        assert ac.long_rows(R, Npix) and not ac.long_rows(R, 2 * Nc)
    assert b0[2] % 2 == 0 and b0[2] % 4 == 2 and b1[2] % 2 == 1          # ring kernel with misaligned rows / register-staged
    for c in (b2, b3):
        assert not ac.long_rows(c[0], c[2]) and c[0] == b0[0] and 0 < b0[2] - c[2] < 8
    assert b2[2] % 2 == 0 and b3[2] % 2 == 1
    R, Nc, Npix = f0[:3]
    assert ac.long_rows(R, 2 * Nc) and not ac.long_rows(R, Npix) and (2 * Nc) % 4 == 2 and ac.rpad(R) > R
    assert not ac.long_rows(f1[0], 2 * f1[1]) and f1[0] == R and 0 < Nc - f1[1] < 8
    assert max(c[1] * c[2] * 8 for c in ALL) < 17 << 20                  # the largest Ylm: about 16 MB
    # rows of the tiled split that exist only as padding, and a ragged granule tail, in both directions
    assert ac.rpad(b0[0]) - b0[0] == 63 and (2 * ac.ksteps(b0[2])) % 32 != 0
    assert (2 * ac.ksteps(2 * f0[1])) % 32 != 0


@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_plan_query_agrees_with_the_restated_formulas(case):
    R, Nc, Npix = case[:3]
    for mode, (prec, split, packed) in ac.MODES.items():
        dtype, ys = (1, 0.0) if prec == 'f64' else (0, 4.0 if split else 0.0)
        for direction in (0, 1):
            rc, p = plan(dtype, ys, R, Nc, Npix, direction, int(packed))
            assert rc == 0, (mode, direction)
            fam, MT, rt, ct, S, lng = p
            L = Npix if direction else 2 * Nc
            if mode == 'f64':
                assert (fam, MT, S, lng) == (ac.F64_VALU, 0, 1, 0)
                assert (rt, ct) == (((R + 7) // 8, (Nc + 3) // 4) if direction else ((R + 15) // 16, (Npix + 255) // 256))
                continue
            assert MT == ac.mt(R) and rt == ac.rpad(R) // (MT * 32)
            if mode == 'exact':
                assert fam == ac.F32_MFMA and lng == 0
                assert ct == ((Nc + 15) // 16 if direction else (Npix + 127) // 128)
                assert S == (ac.exact_bwd_splits(R, Nc, Npix) if direction else 1)
                continue
            assert lng == int(ac.long_rows(R, L))
            assert 1 <= S <= (ac.bwd_max_splits(Npix) if direction else max(1, ac.fwd_packed_chunks(Nc)))
            if not direction:
                assert fam == (ac.PACKED4 if packed else ac.F16_REG) and ct == (Npix + 127) // 128
                assert packed or S == 1
            elif packed:                               # (the default of RIME_ALM_BWD_WIDE: the 8-wave kernel above 64 rows)
                assert fam == (ac.PACKED8 if R > 64 else ac.PACKED4)
                assert ct == ((Nc + 255) // 256 if R > 64 else (Nc + 127) // 128)
            else:                                      # (the default of RIME_ALM_BWD_DMA: the ring at even pixel counts)
                assert fam == (ac.F16_DMA if Npix % 2 == 0 else ac.F16_REG) and ct == (Nc + 127) // 128


def test_forced_split_counts_are_the_counts_in_force(monkeypatch):
    from bayeslim_amd import _lib
    for R, Nc, Npix in ac.FORCED_BWD:
        assert ac.ksteps(Npix) == 104 and ac.bwd_max_splits(Npix) == 3
        assert ac.bwd_chunks(Npix, False) == 52 and ac.bwd_chunks(Npix, True) == 104
        assert ac.deal(52, 3) == [18, 17, 17] and ac.deal(52, 2) == [26, 26] and ac.deal(104, 3) == [35, 35, 34]
        for S in ac.FORCED_S:
            monkeypatch.setenv('RIME_ALM_BWD_SPLITS', str(S))
            for packed in (0, 1):
                rc, p = plan(0, 4.0, R, Nc, Npix, 1, packed)
                assert rc == 0 and p[4] == S, (R, Npix, S, packed, p)
            # the exact-f32 planner has no such switch, and the workspace query sizes the S partial planes
            assert plan(0, 0.0, R, Nc, Npix, 1, 0)[1][4] == ac.exact_bwd_splits(R, Nc, Npix) == 1
            assert _lib.lib.rime_alm2pix_bwd_workspace(0, R, Nc, Npix) >= S * R * Nc * 8
        monkeypatch.delenv('RIME_ALM_BWD_SPLITS')
    for R, Nc, Npix in ac.FORCED_FWD:
        assert ac.fwd_packed_chunks(Nc) == 4
        assert ac.fwd_packed_deal(Nc, 3) == [2, 2, 0] and ac.fwd_packed_deal(Nc, 2) == [2, 2] and ac.fwd_packed_deal(Nc, 1) == [4]
        base = None
        for S in ac.FORCED_S:
            monkeypatch.setenv('RIME_ALM_FWD_SPLITS', str(S))
            rc, p = plan(0, 4.0, R, Nc, Npix, 0, 1)
            assert rc == 0 and p[4] == S and p[0] == ac.PACKED4
            assert plan(0, 4.0, R, Nc, Npix, 0, 0)[1][4] == 1              # the unpacked forward never splits K
            ws = _lib.lib.rime_alm2pix_fwd_workspace(0, R, Nc, Npix)
            base = ws if S == 1 else base
            assert ws == base + (S * R * Npix * 4 if S > 1 else 0)
        monkeypatch.delenv('RIME_ALM_FWD_SPLITS')
    # the exact-f32 backward splits pixels only from 2048 pixels on: the long-row cases reach S > 1 there
    R, Nc, Npix = ac.LONG_CASES[0][:3]
    assert ac.exact_bwd_splits(R, Nc, Npix) == 15 == plan(0, 0.0, R, Nc, Npix, 1, 0)[1][4]


def test_plan_query_refuses_bad_arguments():
    from bayeslim_amd import _lib
    ok = (0, 4.0, 8, 8, 8, 0, 0)
    assert plan(*ok)[0] == 0
    for k, bad in ((0, 2), (0, -1), (1, -1.0), (1, float('nan')), (2, 0), (3, 0), (4, 0), (2, -5), (5, 2), (5, -1), (6, 2), (6, -1)):
        args = list(ok)
        args[k] = bad
        rc, p = plan(*args)
        assert rc == -1 and p == [-7] * 6, (k, bad)
    assert plan(1, 4.0, 8, 8, 8, 0, 1)[0] == -1              # packed: float32 only
    assert plan(0, 0.0, 8, 8, 8, 1, 1)[0] == -1              # packed: the f16 split only
    assert _lib.lib.rime_alm2pix_plan(0, 4.0, 8, 8, 8, 0, 0, None) == -1
    assert _lib.SIGNATURES['rime_alm2pix_plan'] == (ctypes.c_int, [ctypes.c_int, ctypes.c_double] + [ctypes.c_int] * 5
                                                   + [ctypes.POINTER(ctypes.c_int)])


# ---------------------------------------------------------------------------------------------- the bound
def test_split_f16_is_the_f16_grid_toward_zero():
    x = np.array([1.0, ac.XS, -ac.XS, 2.0 ** -14, 2.0 ** -14 * (1 + 2.0 ** -10), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -24 + 2.0 ** -30,
                  8191.99951171875, 0.0, 1 / 3], dtype=np.float32).astype(np.float64)
    hi, lo = ac.split_f16(x)
    h16 = hi.astype(np.float16).astype(np.float64)
    assert (h16 == hi).all() and (lo.astype(np.float16).astype(np.float64) == lo).all()      # both on the f16 grid
    assert (np.abs(hi) <= np.abs(x)).all() and (np.abs(hi + lo) <= np.abs(x)).all()
    assert (np.abs(x - hi) < np.maximum(2.0 ** -10 * np.abs(x), 2.0 ** -24)).all() or (x == hi).all()
    assert (np.abs(x - hi - lo) <= np.maximum(2.0 ** -20 * np.abs(x), 2.0 ** -24)).all()
    assert hi[1] == 1.0 and abs(lo[1] / x[1] - 0.9985 * 2.0 ** -10) < 1e-3 * 2.0 ** -10       # XS: the largest lo image
    assert hi[6] == 0 and lo[6] == 0 and hi[7] == 3 * 2.0 ** -24 and lo[7] == 0


def test_row_scale_restates_the_kernel():
    X = np.zeros((6, 4), np.float32)
    X[0] = [1, -3, 2, 0]              # max 3: 8192 / 3 = 2730.7 -> 2^11
    X[1, 2] = 8192                    # 2^0
    X[2, 0] = 2.0 ** -120             # 2^133 -> clamped to 2^100
    X[3, 1] = 2.0 ** 120              # 2^-107 -> clamped to 2^-100
    X[5, 3] = ac.XS                   # 2^12
    s = ac.row_scale(X)
    assert list(s) == [2.0 ** 11, 1.0, 2.0 ** 100, 2.0 ** -100, 1.0, 2.0 ** 12]
    ok = (s != 1) & (np.abs(np.log2(s)) < 100)
    m = np.abs(X).max(1)[ok] * s[ok]
    assert ((m >= 2.0 ** 12) & (m < 2.0 ** 13)).all()


def operands(case, direction):
    """A [R, K], B [K, N] per real sum of one direction, with S, the 1-norms, the row scales and the float64 reference"""
    R, Nc, Npix = case[:3]
    d = ac.case_data(R, Nc, Npix, 'f32')
    if direction == 0:
        A, Yk = ac.real_operands(d['alm'], d['Y'], np.float64)
        ref, S, asum, ysum = d['fwd']
        return [(A, Yk, ref, S, asum, ysum, d['srow_fwd'], d['ys'])]
    (re, im), S, gsum, ysum = d['bwd']
    g = d['gout'].astype(np.float64)
    return [(g, d['Y'].real.astype(np.float64).T, re, S.real, gsum, ysum.real, d['srow_bwd'], d['ys']),
            (g, -d['Y'].imag.astype(np.float64).T, im, S.imag, gsum, ysum.imag, d['srow_bwd'], d['ys'])]


@pytest.mark.parametrize('direction', [0, 1], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_emulated_split_stays_inside_the_bound_and_faults_leave_it(case, direction):
    for A, B, ref, S, asum, ysum, srow, ys in operands(case, direction):
        K = A.shape[1]
        bsplit = ac.bound_split(S, asum, ysum, srow, ys)
        full = ac.bound(S, K, 'f32', (asum, ysum, srow, ys))
        err = np.abs(ac.emulate(A, B, srow, ys) - ref)
        with np.errstate(divide='ignore', invalid='ignore'):
            worst = np.where(err > 0, err / bsplit, 0).max()
        print('%s dir %d K %d: emulated split error / split part of the bound %.3f' % (ac.case_id(case), direction, K, worst))
        assert worst <= 1.0
        for fault in ('a_lo', 'b_lo', 'scale', 'tail'):
            if fault.endswith('lo') and K > LO_VISIBLE_K:
                continue
            err = np.abs(ac.emulate(A, B, srow, ys, lose=fault) - ref)
            with np.errstate(divide='ignore', invalid='ignore'):
                worst = np.where(err > 0, err / full, 0).max()
            print('    fault %-5s: error / bound %.3g' % (fault, worst))
            assert worst > 1.0, fault


def test_lost_lo_images_are_checked_wherever_the_bound_can_see_them():
    """the one place the accumulation term swallows a lost lo image is the forward of the long-row forward cases"""
    skipped = [(ac.case_id(c), d) for c in ALL for d in (0, 1) if (c[2] if d else 2 * c[1]) > LO_VISIBLE_K]
    assert skipped == [(ac.case_id(c), 0) for c in ac.LONG_CASES[4:]]
    assert (LO_VISIBLE_K + ac.C_RED + 48 + 4) * 2.0 ** -24 < 0.9985 * 2.0 ** -10


def test_reference_is_the_formula_of_the_kernel_file():
    """the real-GEMM restatement against the complex formula, on a small case in exact rational-free float64"""
    alm, Y, gout = ac.draw(5, 3, 7, 'f64', seed=1)
    out, S, _, _ = ac.forward(alm, Y, 'f64')
    assert np.allclose(np.asarray(out, np.float64), (alm @ Y).real, rtol=1e-13, atol=0)
    (re, im), S, _, _ = ac.backward(gout, Y, 'f64')
    want = gout @ Y.conj().T
    scale = np.abs(gout) @ np.abs(Y).T
    assert (np.abs(np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64) - want) <= 1e-13 * scale).all()
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, 'the float64 path needs a reference finer than float64'
