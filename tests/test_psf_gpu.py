"""
The fused phasor-Gram kernel of the full PSF matrix (csrc/psf.hip, ops.psf_gram) on the GPU against the float64
restatement of psf_common.py, and imaging.compute_P / VisMapper on it against the reference's recorded outputs
(tests/golden/psf.npz).  One tolerance throughout: relmax (max abs difference over max abs reference) below 1e-10 in
float64 and 2e-5 in float32, the imaging tolerances of this project.  Shapes follow the kernel's tile and chunk sizes.
"""
import functools

import numpy as np
import pytest
import torch

import psf_common as pc
from conftest import load_golden
from test_rime_gpu import T, DEV, make_array, pixbeam_from_golden, _profiled, ba, prec  # noqa: F401  (ba, prec: fixtures)
from bayeslim_amd import ops

pytestmark = pytest.mark.gpu
TL, CH = ops.PSF_TILE, ops.PSF_BCHUNK
SHAPES = pc.shapes(TL, CH, ops.PSF_FLUSH)
RECT = pc.rect_shapes(TL)
DT = {'f64': torch.float64, 'f32': torch.float32}


@pytest.fixture(params=['f64', 'f32'])
def dt(request):
    return request.param


@functools.lru_cache(maxsize=None)
def problem(seed, Nbl, Nf, P, Pq=None, w_per_channel=True):
    return pc.problem(seed, Nbl, Nf, P, Pq, w_per_channel)


@functools.lru_cache(maxsize=None)
def reference(seed, Nbl, Nf, P, Pq=None, w_per_channel=True, scaled=False):
    """the restatement of a problem, computed once and shared (never modified: the tests only read it)"""
    p = problem(seed, Nbl, Nf, P, Pq, w_per_channel)
    return pc.psf(p['blvecs'], p['freqs'], p['w'], p['s'], p.get('t'), p['rs'] if scaled else None, p['cs'] if scaled else None)


def geometry(p, key='s'):
    s = p[key]
    sdir = torch.zeros(1, 3, ops.pad_to_tile(s.shape[1]), dtype=torch.float64, device=DEV)
    sdir[0, :, :s.shape[1]] = s.to(DEV)
    geom = ops.FringeGeometry(p['blvecs'].to(DEV), sdir, p['freqs'], npix=[s.shape[1]], mfma=False)
    geom.P = s.shape[1]
    return geom


def dev(x, dt):
    return x.to(DT[dt]).to(DEV)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'P%d-Nbl%d-Nf%d-%s' % (s[0], s[1], s[2], 'wf' if s[3] else 'w1'))
def test_symmetric_form_against_the_restatement(shape, dt):
    P, Nbl, Nf, wf = shape
    key = (11, Nbl, Nf, P, None, wf)
    p = problem(*key)
    out = ops.psf_gram(geometry(p), dev(p['w'], dt))
    assert out.shape == (Nf, P, P) and out.dtype == DT[dt]
    err = pc.relmax(out, reference(*key))
    print('symmetric %s %s: relmax %.3e' % (shape, dt, err))
    assert err < pc.TOL[dt]
    assert torch.equal(out, out.transpose(-1, -2))                 # no scales: bitwise symmetric


def test_mirrored_tiles_carry_swapped_scales(dt):
    key = (12, 2 * CH + 5, 3, 2 * TL + 3, None, True)
    p = problem(*key)
    out = ops.psf_gram(geometry(p), dev(p['w'], dt), rs=dev(p['rs'], dt), cs=dev(p['cs'], dt))
    ref = reference(*key, scaled=True)
    assert pc.relmax(ref, ref.transpose(-1, -2)) > 0.1             # rs != cs: the matrix is far from symmetric
    err = pc.relmax(out, ref)
    print('scaled symmetric %s: relmax %.3e' % (dt, err))
    assert err < pc.TOL[dt]
    lower = torch.tril(torch.ones(out.shape[-2:], dtype=torch.bool), -1)
    assert pc.relmax(out.cpu()[:, lower], ref[:, lower]) < pc.TOL[dt]                 # the mirrored half on its own
    only_rs = ops.psf_gram(geometry(p), dev(p['w'], dt), rs=dev(p['rs'], dt))
    assert pc.relmax(only_rs, reference(*key) * p['rs'][:, :, None]) < pc.TOL[dt]


@pytest.mark.parametrize('PPq', RECT, ids=lambda s: 'P%d-Pq%d' % s)
def test_rectangular_form_against_the_restatement(PPq, dt):
    P, Pq = PPq
    key = (13, CH + 1, 3, P, Pq, True)
    p = problem(*key)
    gr, gq = geometry(p), geometry(p, 't')
    out = ops.psf_gram(gr, dev(p['w'], dt), rs=dev(p['rs'], dt), cs=dev(p['cs'], dt), geom_q=gq)
    assert out.shape == (3, P, Pq)
    err = pc.relmax(out, reference(*key, scaled=True))
    print('rectangular %s %s: relmax %.3e' % (PPq, dt, err))
    assert err < pc.TOL[dt]


def test_rectangular_form_over_the_rows_equals_the_symmetric_form(dt):
    key = (14, CH + 1, 3, TL + 1, None, True)
    p = problem(*key)
    sym = ops.psf_gram(geometry(p), dev(p['w'], dt))
    rect = ops.psf_gram(geometry(p), dev(p['w'], dt), geom_q=geometry(p))
    assert pc.relmax(rect, reference(*key)) < pc.TOL[dt] and pc.relmax(rect, sym.cpu().numpy()) < pc.TOL[dt]


def test_index_maps_and_accumulation(dt):
    n, L, Nf, Nbl = TL + 5, 2 * TL + 7, 3, CH + 1
    key = (15, Nbl, Nf, n, 9, True)
    p = problem(*key)
    gen = torch.Generator().manual_seed(5)
    rows = torch.randperm(L, generator=gen)[:n]
    cols9 = torch.randperm(L, generator=gen)[:9]
    pattern = (torch.arange(Nf * L * L, dtype=torch.float64).reshape(Nf, L, L) % 17 - 8.0) * 0.37
    w1, w2 = p['w'], p['w'].flip(0) * 1.5
    S1 = pc.psf(p['blvecs'], p['freqs'], w1, p['s'])
    S2 = pc.psf(p['blvecs'], p['freqs'], w2, p['s'])
    out = dev(pattern, dt).contiguous()
    start = out.clone()
    geom = geometry(p)
    assert ops.psf_gram(geom, dev(w1, dt), out=out, rows=rows.to(DEV), cols=rows.to(DEV), accumulate=True) is out
    ops.psf_gram(geom, dev(w2, dt), out=out, rows=rows, cols=rows.to(torch.int32), accumulate=True)
    ref = start.cpu().double()
    ref[:, rows[:, None], rows[None, :]] += S1 + S2
    touched = torch.zeros(L, L, dtype=torch.bool)
    touched[rows[:, None], rows[None, :]] = True
    assert pc.relmax(out.cpu()[:, touched], ref[:, touched]) < pc.TOL[dt]
    assert torch.equal(out.cpu()[:, ~touched], start.cpu()[:, ~touched])              # untouched: the same bits
    # accumulate=False overwrites what it owns and nothing else
    ops.psf_gram(geom, dev(w1, dt), out=out, rows=rows, cols=rows)
    ref[:, rows[:, None], rows[None, :]] = S1
    assert pc.relmax(out.cpu()[:, touched], ref[:, touched]) < pc.TOL[dt]
    assert torch.equal(out.cpu()[:, ~touched], start.cpu()[:, ~touched])
    # rectangular form, rows != cols
    out = start.clone()
    R = pc.psf(p['blvecs'], p['freqs'], w1, p['s'], p['t'], p['rs'], p['cs'])
    ops.psf_gram(geom, dev(w1, dt), rs=dev(p['rs'], dt), cs=dev(p['cs'], dt), geom_q=geometry(p, 't'), out=out, rows=rows,
                 cols=cols9, accumulate=True)
    ref = start.cpu().double()
    ref[:, rows[:, None], cols9[None, :]] += R
    touched = torch.zeros(L, L, dtype=torch.bool)
    touched[rows[:, None], cols9[None, :]] = True
    assert pc.relmax(out.cpu()[:, touched], ref[:, touched]) < pc.TOL[dt]
    assert torch.equal(out.cpu()[:, ~touched], start.cpu()[:, ~touched])


def test_run_to_run_determinism(dt):
    p = problem(16, 2 * CH + 5, 3, 2 * TL + 3, TL - 1, True)
    geom, gq, w = geometry(p), geometry(p, 't'), dev(p['w'], dt)
    rs, cs = dev(p['rs'], dt), dev(p['cs'], dt)
    assert torch.equal(ops.psf_gram(geom, w, rs=rs, cs=rs), ops.psf_gram(geom, w, rs=rs, cs=rs))
    assert torch.equal(ops.psf_gram(geom, w, rs=rs, cs=cs, geom_q=gq), ops.psf_gram(geom, w, rs=rs, cs=cs, geom_q=gq))


def test_other_stream_gives_the_same_bits(dt):
    p = problem(16, 2 * CH + 5, 3, 2 * TL + 3, TL - 1, True)
    geom, w = geometry(p), dev(p['w'], dt)
    base = ops.psf_gram(geom, w)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        other = ops.psf_gram(geom, w)
    stream.synchronize()
    assert torch.equal(base, other)


def test_module_compute_P_against_the_reference(ba, prec):
    from bayeslim_amd import imaging
    g = load_golden('psf')
    geom = imaging.geometry(T(g['one_blvecs'], torch.float64), g['one_zen'], g['one_az'], torch.as_tensor(g['freqs']))
    P, kernels = _profiled(ops, lambda: imaging.compute_P(geom, T(g['one_w']), T(g['one_beam']), T(g['one_D']), contract=None))
    assert kernels == ['psf_gram_kernel'] and P.shape == (2, 37, 37)
    assert pc.relmax(P, g['one_P']) < pc.TOL[prec]
    sub = [3, 20, 36]
    gq = imaging.geometry(T(g['one_blvecs'], torch.float64), g['one_zen'][sub], g['one_az'][sub], torch.as_tensor(g['freqs']))
    Pq = imaging.compute_P(geom, T(g['one_w']), T(g['one_beam']), T(g['one_D']), geom_q=gq, beam_q=T(g['one_beam'])[:, sub])
    assert Pq.shape == (2, 37, 3) and pc.relmax(Pq, g['one_P'][:, :, sub]) < pc.TOL[prec]


def test_vismapper_full_psf_against_the_reference(ba, prec):
    """the reference's VisMapper of make_golden_psf.py: Airy PixelBeam, fov 120, 2 times whose cuts differ, supplied icov"""
    from bayeslim_amd import imaging, dataset
    g = load_golden('psf')
    tol = pc.TOL[prec]
    freqs = T(g['freqs'])
    arr, tel = make_array(ba, g, freqs)
    vd = dataset.VisData()
    vd.setup_meta(tel, arr.to_antpos())
    vd.setup_data([tuple(b) for b in g['bls'].tolist()], torch.as_tensor(g['times']), freqs, pol='ee', data=T(g['data']))
    beam = pixbeam_from_golden(ba, g, freqs, parameter=False)
    beam.fov = 120
    Npix = len(g['ra'])
    vm = imaging.VisMapper(vd, g['ra'], g['dec'], beam=beam)
    for t, za in zip(g['times'], g['zenaz']):
        vm.telescope.conv_cache[(float(t), Npix)] = torch.as_tensor(za, dtype=torch.float64)
    vm.set_normalization('A2w', icov=T(g['icov']))
    maps, P = vm.make_map(return_P=True, contract=None)
    assert P.shape == (2, Npix, Npix)
    assert pc.relmax(maps, g['maps']) < tol and pc.relmax(P, g['P']) < tol and pc.relmax(vm.D, g['D']) < tol
    Pc, kernels = _profiled(ops, lambda: vm.compute_P(contract=None))
    assert pc.relmax(Pc, g['P_compute']) < tol
    assert kernels == ['psf_gram_kernel'] * 2, kernels             # one launch per time step, no fringe_* launch
    # columns of it: a pixel of both cuts, one of the second cut only, one of the first only, one of neither
    c0, c1 = set(g['cut0'].tolist()), set(g['cut1'].tolist())
    k = [sorted(c0 & c1)[2], sorted(c1 - c0)[0], sorted(c0 - c1)[0], sorted(set(range(Npix)) - c0 - c1)[0], sorted(c0 & c1)[0]]
    Pk, kernels = _profiled(ops, lambda: vm.compute_P(contract=None, pix_inds=k))
    assert Pk.shape == (2, Npix, 5) and kernels == ['psf_gram_kernel'] * 2
    assert pc.relmax(Pk, g['P_compute'][:, :, k]) < tol and float(Pk[:, :, 3].abs().max()) == 0.0
    assert torch.equal(vm.compute_P(contract=None, pix_inds=torch.as_tensor(k[:1]))[:, :, 0], Pk[:, :, 0])
    with pytest.raises(ValueError, match='contract must be None'):
        vm.compute_P(contract='diag', pix_inds=k)
    with pytest.raises(ValueError, match='unique pixel indices'):
        vm.compute_P(contract=None, pix_inds=[1, 1])
