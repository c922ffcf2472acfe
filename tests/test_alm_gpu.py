"""
GPU checks of csrc/alm.hip (ops.alm2pix with its adjoint, and the C entry points directly) against the restatement of
tests/alm_common.py: every case of its table in four modes -- complex128, complex64 on the exact-f32 matrix cores
(ops.ALM_SPLIT_F16 = False), complex64 f16-split unpacked and packed (ops.ALM_PACKED_MIN_BYTES = 0) -- elementwise at the
bound derived there, run twice with equal bits.  rime_alm2pix_plan says which kernel family, MT, grid and split count every
case ran, and test_cases_reach_every_kernel asserts the table leaves none out.  tests/test_alm_host.py shows without a GPU
that the bound notices a lost lo image, a wrong row scale and a dropped K tail.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import alm_common as ac

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
HERE = os.path.dirname(os.path.abspath(__file__))
ALL = ac.CASES + ac.LONG_CASES
IDS = [ac.case_id(c) for c in ALL]
WORST = {}                       # (mode, direction) -> worst error / bound seen, printed by the last test


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from bayeslim_amd import ops as _ops
    return _ops


def dev(x):
    return torch.as_tensor(np.array(x)).to(DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def plan(ops, mode, R, Nc, Npix, direction):
    prec, split, packed = ac.MODES[mode]
    out = (ctypes.c_int * 6)()
    rc = ops.lib.rime_alm2pix_plan(1 if prec == 'f64' else 0, 4.0 if split else 0.0, R, Nc, Npix, direction, int(packed), out)
    assert rc == 0
    return tuple(out)


def set_mode(ops, monkeypatch, mode):
    prec, split, packed = ac.MODES[mode]
    monkeypatch.setattr(ops, 'ALM_SPLIT_F16', split)
    monkeypatch.setattr(ops, 'ALM_PACKED', packed)
    monkeypatch.setattr(ops, 'ALM_PACKED_MIN_BYTES', 0)
    return prec, split, packed


def run_twice(ops, alm, Y, gout, packed=False):
    """forward and adjoint through ops.alm2pix, twice: equal bits (NaN-free by the checks that follow)"""
    res = []
    for _ in range(2):
        x = alm.clone().requires_grad_(True)
        y = ops.alm2pix(x, Y)
        g, = torch.autograd.grad(y, x, gout)
        res.append((y.detach(), g))
    for a, b in zip(res[0], res[1]):
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
        assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                           b.view(torch.int64 if b.dtype == torch.float64 else torch.int32)), 'two runs, different bits'
    if packed:
        st = ops.ylm_packed_state(Y)
        assert st is not None and all(st[3].get(k) not in (None, False) for k in (0, 1)), 'the packed copies were not used'
    return res[0][0].cpu().numpy(), res[0][1].cpu().numpy()


def note(mode, direction, worst):
    WORST[(mode, direction)] = max(WORST.get((mode, direction), 0.0), worst)


# ------------------------------------------------------------------------------------- 1. accuracy and determinism
@pytest.mark.parametrize('mode', list(ac.MODES))
@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_every_case_against_the_reference(ops, monkeypatch, case, mode):
    R, Nc, Npix = case[:3]
    prec, split, packed = set_mode(ops, monkeypatch, mode)
    d = ac.case_data(R, Nc, Npix, prec)
    Y = dev(d['Y'])
    out, galm = run_twice(ops, dev(d['alm']), Y, dev(d['gout']), packed)
    if split:
        assert ops._ylm_scale(Y) == d['ys']
    what = '%s %s' % (ac.case_id(case), mode)
    for direction in (0, 1):
        p = plan(ops, mode, R, Nc, Npix, direction)
        print('%s %s: %s, MT %d, %d row x %d column tiles, S %d, long rows %d' % ((what, 'bwd' if direction else 'fwd', ac.FAMILY[p[0]]) + p[1:]))
    note(mode, 0, ac.check_forward(out, d, 2 * Nc, prec, split, what))
    note(mode, 1, ac.check_backward(galm, d, Npix, prec, split, what))


# ------------------------------------------------------------------------------------- 2. coverage
def test_cases_reach_every_kernel(ops, monkeypatch):
    seen = {}                                # (direction, family, MT) -> [max row tiles, max S, long rows seen]
    def add(mode, R, Nc, Npix):
        for direction in (0, 1):
            fam, MT, rt, ct, S, lng = plan(ops, mode, R, Nc, Npix, direction)
            e = seen.setdefault((direction, fam, MT), [0, 0, 0])
            e[0], e[1], e[2] = max(e[0], rt), max(e[1], S), max(e[2], lng)
    for c in ALL:
        for mode in ac.MODES:
            add(mode, *c[:3])
    for S in ac.FORCED_S:
        monkeypatch.setenv('RIME_ALM_BWD_SPLITS', str(S))
        monkeypatch.setenv('RIME_ALM_FWD_SPLITS', str(S))
        for c in ac.FORCED_BWD + ac.FORCED_FWD:
            add('split', *c)
            add('packed', *c)
    for k in sorted(seen):
        print('%s %-26s MT %d: row tiles up to %d, S up to %d, long rows %d' % (('bwd' if k[0] else 'fwd', ac.FAMILY[k[1]], k[2]) + tuple(seen[k])))
    # every family x MT one process can reach (RIME_ALM_BWD_WIDE=0 / _DMA=0: tests/alm_switch_child.py)
    want = {(0, ac.F64_VALU, 0), (1, ac.F64_VALU, 0)}
    for MT in (1, 2, 4):
        want |= {(0, ac.F32_MFMA, MT), (1, ac.F32_MFMA, MT), (0, ac.F16_REG, MT), (1, ac.F16_REG, MT), (1, ac.F16_DMA, MT), (0, ac.PACKED4, MT)}
    want |= {(1, ac.PACKED4, 1), (1, ac.PACKED4, 2), (1, ac.PACKED8, 4)}
    assert set(seen) == want
    # more than one row tile in every family whose rows can exceed a tile in this process (the 4-wave packed backward
    # serves at most 64 rows here: one tile of MT 2)
    for k in seen:
        if k[2] in (0, 4):
            assert seen[k][0] > 1, k
    # S > 1 in every family that splits, and the forced count 3 in every family that reads the switches
    assert seen[(1, ac.F32_MFMA, 4)][1] > 1
    assert seen[(0, ac.PACKED4, 4)][1] == 3
    for k in ((1, ac.F16_REG, 2), (1, ac.F16_DMA, 2), (1, ac.PACKED4, 2), (1, ac.F16_REG, 4), (1, ac.F16_DMA, 4), (1, ac.PACKED8, 4)):
        assert seen[k][1] >= 3, k
    # the long-row split in both directions, unpacked and packed
    assert seen[(0, ac.F16_REG, 2)][2] and seen[(0, ac.PACKED4, 2)][2]
    assert seen[(1, ac.F16_REG, 4)][2] and seen[(1, ac.F16_DMA, 4)][2] and seen[(1, ac.PACKED8, 4)][2]


# ------------------------------------------------------------------------------------- 3. direct calls, poisoned buffers
def direct(ops, direction, packed, d, R, Nc, Npix):
    """one transform through the C entry points: workspace of exactly the queried size filled with 0xFF bytes (NaN as
    float32), the packed buffer likewise before packing, the output pre-filled with NaN"""
    lib, ys = ops.lib, d['ys']
    Y = torch.view_as_real(dev(d['Y'])).contiguous()
    nws = int((lib.rime_alm2pix_bwd_workspace if direction else lib.rime_alm2pix_fwd_workspace)(0, R, Nc, Npix))
    assert nws > 0
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=DEV)
    if direction:
        x = dev(d['gout'])
        out = torch.full((R, Nc, 2), float('nan'), dtype=torch.float32, device=DEV)
    else:
        x = torch.view_as_real(dev(d['alm'])).contiguous()
        out = torch.full((R, Npix), float('nan'), dtype=torch.float32, device=DEV)
    if packed:
        nb = int(lib.rime_alm2pix_packed_bytes(Nc, Npix, direction))
        buf = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
        assert lib.rime_alm2pix_pack(ptr(Y), ys, Nc, Npix, direction, ptr(buf), stream()) == 0
        f = lib.rime_alm2pix_bwd_packed if direction else lib.rime_alm2pix_fwd_packed
        rc = f(ptr(x), ptr(buf), ys, R, Nc, Npix, ptr(out), ptr(ws), nws, stream())
    else:
        f = lib.rime_alm2pix_bwd if direction else lib.rime_alm2pix_fwd
        rc = f(0, ptr(x), ptr(Y), ys, R, Nc, Npix, ptr(out), ptr(ws), nws, stream())
    assert rc == 0, ops.lib.rime_last_error()
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.isfinite(res).all(), 'an output element was not written, or unwritten workspace leaked into it'
    return res[..., 0] + 1j * res[..., 1] if direction else res


def check_direct(ops, direction, packed, R, Nc, Npix, what):
    d = ac.case_data(R, Nc, Npix, 'f32')
    a, b = (direct(ops, direction, packed, d, R, Nc, Npix) for _ in range(2))
    assert a.tobytes() == b.tobytes(), 'two runs, different bits'
    if direction:
        return a, ac.check_backward(a, d, Npix, 'f32', True, what)
    return a, ac.check_forward(a, d, 2 * Nc, 'f32', True, what)


@pytest.mark.parametrize('S', ac.FORCED_S)
@pytest.mark.parametrize('shape', ac.FORCED_BWD, ids=ac.case_id)
def test_forced_backward_splits(ops, monkeypatch, shape, S):
    R, Nc, Npix = shape
    monkeypatch.setenv('RIME_ALM_BWD_SPLITS', str(S))
    res = {}
    for packed, mode in ((0, 'split'), (1, 'packed')):
        p = plan(ops, mode, R, Nc, Npix, 1)
        assert p[4] == S
        wide = p[0] == ac.PACKED8
        dealt = ac.deal(ac.bwd_chunks(Npix, wide), S)
        print('%s %s S %d: %s, chunks per split %s' % (ac.case_id(shape), mode, S, ac.FAMILY[p[0]], dealt))
        assert dealt == {(False, 1): [52], (False, 2): [26, 26], (False, 3): [18, 17, 17],
                         (True, 1): [104], (True, 2): [52, 52], (True, 3): [35, 35, 34]}[(wide, S)]
        res[mode], w = check_direct(ops, 1, packed, R, Nc, Npix, '%s %s S=%d' % (ac.case_id(shape), mode, S))
        note(mode, 1, w)


@pytest.mark.parametrize('S', ac.FORCED_S)
@pytest.mark.parametrize('shape', ac.FORCED_FWD, ids=ac.case_id)
def test_forced_forward_splits_with_an_empty_split(ops, monkeypatch, shape, S):
    R, Nc, Npix = shape
    monkeypatch.setenv('RIME_ALM_FWD_SPLITS', str(S))
    assert plan(ops, 'packed', R, Nc, Npix, 0)[4] == S
    dealt = ac.fwd_packed_deal(Nc, S)
    assert dealt == {1: [4], 2: [2, 2], 3: [2, 2, 0]}[S]                     # S = 3: the third split's plane is all zeros
    got, w = check_direct(ops, 0, 1, R, Nc, Npix, '%s packed S=%d' % (ac.case_id(shape), S))
    note('packed', 0, w)
    if S == 1:                                                               # no K split: the unpacked kernel's bits
        ref, _ = check_direct(ops, 0, 0, R, Nc, Npix, '%s split' % ac.case_id(shape))
        assert got.tobytes() == ref.tobytes()


@pytest.mark.parametrize('packed', [0, 1], ids=['split', 'packed'])
@pytest.mark.parametrize('case', ac.LONG_CASES, ids=ac.case_id)
def test_long_rows_through_the_c_entry_points(ops, case, packed):
    R, Nc, Npix = case[:3]
    mode = 'packed' if packed else 'split'
    for direction in (0, 1):
        p = plan(ops, mode, R, Nc, Npix, direction)
        assert p[5] == int(ac.long_rows(R, Npix if direction else 2 * Nc))
        _, w = check_direct(ops, direction, packed, R, Nc, Npix, '%s %s (long rows %d)' % (ac.case_id(case), mode, p[5]))
        note(mode, direction, w)


# ------------------------------------------------------------------------------------- 4. packed against unpacked
@pytest.mark.parametrize('case', ac.CASES, ids=ac.case_id)
def test_packed_against_unpacked(ops, monkeypatch, case):
    R, Nc, Npix = case[:3]
    d = ac.case_data(R, Nc, Npix, 'f32')
    res = {}
    for mode in ('split', 'packed'):
        set_mode(ops, monkeypatch, mode)
        res[mode] = run_twice(ops, dev(d['alm']), dev(d['Y']), dev(d['gout']), mode == 'packed')
    if plan(ops, 'packed', R, Nc, Npix, 0)[4] == 1:
        assert res['split'][0].tobytes() == res['packed'][0].tobytes(), 'forward without a K split: not the same bits'
    (_, _), S, gsum, ysum = d['bwd']
    diff = res['split'][1] - res['packed'][1]
    for got, s, y1 in ((diff.real, S.real, ysum.real), (diff.imag, S.imag, ysum.imag)):
        b = 2 * ac.bound(s, Npix, 'f32', (gsum, y1, d['srow_bwd'], d['ys']))
        assert (np.abs(got.astype(np.float64)) <= b).all()


# ------------------------------------------------------------------------------------- 5. row isolation
@pytest.mark.parametrize('poison', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('mode', ['exact', 'split', 'packed'])
@pytest.mark.parametrize('shape', [(33, 33, 31), (129, 257, 1110), (200, 257, 1111)], ids=ac.case_id)
def test_a_poisoned_row_stays_in_its_row(ops, monkeypatch, shape, mode, poison):
    R, Nc, Npix = shape
    set_mode(ops, monkeypatch, mode)
    d = ac.case_data(R, Nc, Npix, 'f32')
    Y = dev(d['Y'])
    clean = run_twice(ops, dev(d['alm']), Y, dev(d['gout']), mode == 'packed')
    row = R - 2                                                              # in the ragged last row tile where there is one
    alm, gout = np.array(d['alm']), np.array(d['gout'])
    alm[row, Nc // 2] = poison
    gout[row, Npix // 2] = poison
    bad = run_twice_nonfinite(ops, dev(alm), Y, dev(gout))
    keep = np.arange(R) != row
    for c, b in zip(clean, bad):
        assert c[keep].tobytes() == b[keep].tobytes(), 'the poisoned row changed another row'
        assert not np.isfinite(b[row].real).any() and (not np.iscomplexobj(b) or not np.isfinite(b[row].imag).any())


def run_twice_nonfinite(ops, alm, Y, gout):
    x = alm.clone().requires_grad_(True)
    y = ops.alm2pix(x, Y)
    g, = torch.autograd.grad(y, x, gout)
    return y.detach().cpu().numpy(), g.cpu().numpy()


# ------------------------------------------------------------------------------------- 6. switches read once per process
@pytest.fixture(scope='module')
def children(tmp_path_factory):
    d = tmp_path_factory.mktemp('alm_switch')
    out = {}
    for name, env in (('narrow', dict(RIME_ALM_BWD_WIDE='0', RIME_ALM_BWD_DMA='0')), ('default', {})):
        base = {k: v for k, v in os.environ.items() if k not in ('RIME_ALM_BWD_WIDE', 'RIME_ALM_BWD_DMA', 'RIME_ALM_BWD_SPLITS')}
        path = str(d / name)
        r = subprocess.run([sys.executable, os.path.join(HERE, 'alm_switch_child.py'), path], env=dict(base, **env),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, '%s:\n%s\n%s' % (name, r.stdout[-2000:], r.stderr[-4000:])
        with open(path + '.json') as f:
            out[name] = (json.load(f), np.load(path + '.npz'))
    return out


@pytest.mark.parametrize('shape', ac.SWITCH_CASES, ids=ac.case_id)
def test_switched_kernels_hold_the_bound_and_agree_with_the_default_ones(children, shape):
    R, Nc, Npix = shape
    cid = ac.case_id(shape)
    d = ac.case_data(R, Nc, Npix, 'f32')
    (_, _), S, gsum, ysum = d['bwd']
    for mode in ('split', 'packed'):
        key = '%s|%s' % (cid, mode)
        n, w = children['narrow'][0][key], children['default'][0][key]
        print('%s %s: switched off %s (MT %d, S %d) worst %.3f; default %s (MT %d, S %d) worst %.3f' % (
            cid, mode, ac.FAMILY[n['plan'][0]], n['plan'][1], n['plan'][4], n['worst'],
            ac.FAMILY[w['plan'][0]], w['plan'][1], w['plan'][4], w['worst']))
        if mode == 'packed':
            assert n['plan'][:2] == [ac.PACKED4, 4] and w['plan'][:2] == [ac.PACKED8, 4]
            assert n['plan'][2] == (2 if R > 128 else 1)
        else:
            assert n['plan'][:2] == [ac.F16_REG, 4]                          # register-staged also at even pixel counts
            assert w['plan'][:2] == [ac.F16_DMA if Npix % 2 == 0 else ac.F16_REG, 4]
        assert n['worst'] <= 1.0 and w['worst'] <= 1.0 and n['equal_bits'] and w['equal_bits']
        diff = children['narrow'][1][key] - children['default'][1][key]
        for got, s, y1 in ((diff.real, S.real, ysum.real), (diff.imag, S.imag, ysum.imag)):
            b = 2 * ac.bound(s, Npix, 'f32', (gsum, y1, d['srow_bwd'], d['ys']))
            assert (np.abs(got.astype(np.float64)) <= b).all()


def test_print_the_worst_ratio_per_path():
    """(runs last in the file) the figures DESIGN.md 5.3 quotes"""
    for (mode, direction), w in sorted(WORST.items()):
        print('alm2pix %-6s %s: worst error / bound over all cases %.3f' % (mode, 'adjoint' if direction else 'forward', w))
        assert w <= 1.0
