"""
The full-PSF feature without a GPU: imaging.deconvolve_map and imaging.VisData2MapData on the CPU against the reference's
recorded outputs, the restatement of psf_common.py against the reference's module-level compute_P (the yardstick of the
GPU tests checked against the reference), the return codes of the rejected calls of rime_psf_gram, the refusals of
ops.psf_gram, which come before any launch, and the kept assembly of csrc/psf.hip (no scratch, no atomics).
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import kernel_asm
import psf_common as pc
from conftest import load_golden
from bayeslim_amd import _lib, dataset, imaging, ops

F64 = torch.float64


def T(a):
    return torch.as_tensor(np.asarray(a))


def test_restatement_equals_the_reference_compute_P():
    g = load_golden('psf')
    s = pc.pointing_vectors(g['one_zen'], g['one_az'])
    beam, D = T(g['one_beam']), T(g['one_D'])
    P = pc.psf(g['one_blvecs'], g['freqs'], g['one_w'], s, rs=beam * D, cs=beam)
    assert P.shape == g['one_P'].shape == (2, 37, 37)
    assert pc.relmax(P, g['one_P']) < 1e-12


@pytest.mark.parametrize('pinv', [False, True])
def test_deconvolve_map_against_the_reference(pinv):
    g = load_golden('psf')
    dm = imaging.deconvolve_map(T(g['dec_m']), T(g['dec_P']), pinv=pinv)
    ref = g['dec_pinv' if pinv else 'dec_diag']
    assert dm.shape == ref.shape and pc.relmax(dm, ref) < 1e-10
    if pinv:                                                       # a well-conditioned P: the deconvolved map solves P dm = m
        assert pc.relmax(torch.einsum('fpq,fq->fp', T(g['dec_P']), dm), g['dec_m']) < 1e-10


def _flag_vd(g, flags):
    vd = dataset.VisData()
    vd.setup_meta(None, None)
    vd.setup_data([tuple(b) for b in g['md_bls'].tolist()], T(g['times']), T(g['md_freqs']), pol='ee',
                  data=torch.zeros(1, 1, 3, 2, 4, dtype=torch.complex128), flags=flags)
    return vd


def test_visdata2mapdata_against_the_reference():
    """the reference broadcasts the per-channel flags along the PIXEL axis (it runs only for Npix == Nfreqs, see
    make_golden_psf.py); here they lie on the channel axis of (Npol, 1, Nfreqs, Npix), as its own comment states: the
    recorded flags are compared transposed"""
    g = load_golden('psf')
    vd = _flag_vd(g, T(g['md_flags_in']))
    md = imaging.VisData2MapData(vd, data=T(g['md_data']), angs=T(g['md_angs']), norm=T(g['md_norm']), df=torch.full((4,), 1e7),
                                 name='dirty')
    assert isinstance(md, dataset.MapData) and md.name == 'dirty' and md.pols == ['ee']
    assert md.flags.shape == (1, 1, 4, 4) and md.flags.dtype == torch.bool
    assert np.array_equal(md.flags.numpy(), g['md_flags'].swapaxes(-1, -2))
    # flagged if flagged on all baselines and times: channel 1 only (channel 2 is flagged on all but one sample)
    assert md.flags[0, 0, :, 0].tolist() == [False, True, False, False] and bool((md.flags == md.flags[..., :1]).all())
    assert np.array_equal(md.data.numpy(), g['md_out_data']) and np.array_equal(md.norm.numpy(), g['md_out_norm'])
    assert torch.equal(md.freqs, vd.freqs) and torch.equal(md.angs, T(g['md_angs'])) and torch.equal(md.df, torch.full((4,), 1e7))
    # any pixel count (the reference raises here), and no angles: one pixel
    wide = imaging.VisData2MapData(vd, angs=torch.zeros(2, 7))
    assert wide.flags.shape == (1, 1, 4, 7) and wide.flags[0, 0, :, 6].tolist() == [False, True, False, False]
    assert imaging.VisData2MapData(vd).flags.shape == (1, 1, 4, 1)


def test_visdata2mapdata_without_flags_or_pol():
    g = load_golden('psf')
    vd = _flag_vd(g, None)
    md = imaging.VisData2MapData(vd, data=T(g['md_data']), angs=T(g['md_angs']))
    assert md.flags is None and md.pols == ['ee'] and md.data.shape == (1, 1, 4, 4) and md.name is None and md.norm is None
    vd.pol = None
    assert imaging.VisData2MapData(vd).pols == ['ee', 'nn']


# ---- rejected calls (the style of test_icov_host.py): each returns before anything is launched ---------------------------
OK, EINVAL = 0, -1
_BUF = ctypes.create_string_buffer(4096 + 16)
PTR = (ctypes.addressof(_BUF) + 15) & ~15                              # host memory, never dereferenced

BASE = {
    'rime_psf_gram': dict(dtype=0, blvecs=PTR, freqs=PTR, w=PTR, w_sb=3, w_sf=1, Nbl=5, Nf=3, sr=PTR, ld_sr=64, Pr=40, sq=None,
                          ld_sq=0, Pq=0, rs=None, cs=None, rows=None, cols=None, out=PTR, ldr=40, ldc=40, accumulate=0,
                          stream=None),
}
RECT = dict(sq=PTR, ld_sq=64, Pq=7, ldc=7)
ROWS = [
    ('rime_psf_gram', dict(dtype=7), EINVAL), ('rime_psf_gram', dict(dtype=-1), EINVAL),
    ('rime_psf_gram', dict(blvecs=None), EINVAL), ('rime_psf_gram', dict(freqs=None), EINVAL), ('rime_psf_gram', dict(w=None), EINVAL),
    ('rime_psf_gram', dict(sr=None), EINVAL), ('rime_psf_gram', dict(out=None), EINVAL),
    ('rime_psf_gram', dict(Nbl=0), EINVAL), ('rime_psf_gram', dict(Nbl=-3), EINVAL), ('rime_psf_gram', dict(Nf=0), EINVAL),
    ('rime_psf_gram', dict(Nf=65536), EINVAL), ('rime_psf_gram', dict(Pr=0), EINVAL), ('rime_psf_gram', dict(Pr=-1), EINVAL),
    ('rime_psf_gram', dict(RECT, Pq=0), EINVAL), ('rime_psf_gram', dict(RECT, Pq=-2), EINVAL),
    ('rime_psf_gram', dict(ldr=39), EINVAL), ('rime_psf_gram', dict(ldc=39), EINVAL),             # identity maps: smaller than the pixels
    ('rime_psf_gram', dict(RECT, ldc=6), EINVAL), ('rime_psf_gram', dict(rows=PTR, ldr=0), EINVAL),
    ('rime_psf_gram', dict(cols=PTR, ldc=-1), EINVAL),
    ('rime_psf_gram', dict(w_sb=-1), EINVAL), ('rime_psf_gram', dict(w_sf=-1), EINVAL), ('rime_psf_gram', dict(ld_sr=-64), EINVAL),
    ('rime_psf_gram', dict(ld_sr=39), EINVAL), ('rime_psf_gram', dict(RECT, ld_sq=-64), EINVAL), ('rime_psf_gram', dict(RECT, ld_sq=6), EINVAL),
    ('rime_psf_gram', dict(accumulate=2), EINVAL), ('rime_psf_gram', dict(accumulate=-1), EINVAL),
    ('rime_psf_gram', dict(dtype=7, out=None), EINVAL),
]


def _id(row):
    entry, bad, code = row
    return entry[len('rime_'):] + '-' + '-'.join('%s=%s' % (k, 'ptr' if v == PTR else v) for k, v in bad.items())


def test_rejected_call_table_matches_the_signature():
    for entry, args in BASE.items():
        assert len(args) == len(_lib.SIGNATURES[entry][1]), entry
    for entry, bad, code in ROWS:
        assert bad and set(bad) <= set(BASE[entry]) and code != OK
    assert len({_id(r) for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize('row', ROWS, ids=_id)
def test_rejected_call_returns_its_code(row):
    entry, bad, code = row
    args = dict(BASE[entry], **bad)
    assert getattr(_lib.lib, entry)(*args.values()) == code


# ---- the refusals of ops.psf_gram ------------------------------------------------------------------------------------------
def _cpu_geom(Nbl=5, Nf=3, P=6):
    """what psf_gram reads of a FringeGeometry (whose constructor needs a GPU), on the CPU"""
    return types.SimpleNamespace(Nbl=Nbl, Nf=Nf, Nt=1, P=P, Pstride=64, blvecs=torch.zeros(Nbl, 3, dtype=F64),
                                 sdir=torch.zeros(1, 3, 64, dtype=F64), freqs=torch.ones(Nf, dtype=F64))


@pytest.fixture
def no_launch(monkeypatch):
    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError('%s called: the refusal must come before the launch' % name)
    monkeypatch.setattr(ops, 'lib', NoLaunch())


def test_psf_gram_refuses_before_any_launch(no_launch):
    geom, w = _cpu_geom(), torch.ones(5, 3, dtype=F64)
    out = torch.zeros(3, 9, 9, dtype=F64)
    good = torch.tensor([0, 2, 4, 5, 7, 8])
    with pytest.raises(ValueError, match='duplicate'):
        ops.psf_gram(geom, w, out=out, rows=torch.tensor([0, 2, 4, 2, 7, 8]), cols=good, accumulate=True)
    with pytest.raises(ValueError, match='duplicate'):
        ops.psf_gram(geom, w, out=out, rows=good, cols=torch.tensor([1, 1, 2, 3, 4, 5]))
    with pytest.raises(ValueError, match='outside'):
        ops.psf_gram(geom, w, out=out, rows=torch.tensor([0, 2, 4, 5, 7, 9]), cols=good)
    with pytest.raises(ValueError, match='outside'):
        ops.psf_gram(geom, w, out=out, rows=good, cols=torch.tensor([-1, 2, 4, 5, 7, 8]))
    with pytest.raises(ValueError, match='6 integer indices'):
        ops.psf_gram(geom, w, out=out, rows=good[:5], cols=good)
    with pytest.raises(TypeError, match='working dtype'):
        ops.psf_gram(geom, w, out=out.float(), rows=good, cols=good)
    with pytest.raises(ValueError, match='contiguous'):
        ops.psf_gram(geom, w, out=out.transpose(1, 2)[:, :, ::2], rows=None, cols=None)
    with pytest.raises(ValueError, match='smaller'):
        ops.psf_gram(geom, w, out=torch.zeros(3, 5, 9, dtype=F64))
    with pytest.raises(ValueError, match='supplies'):
        ops.psf_gram(geom, w, rows=good, cols=good)
    with pytest.raises(ValueError, match=r'w must be'):
        ops.psf_gram(geom, torch.ones(5, 2, dtype=F64))
    with pytest.raises(TypeError, match='float32 or float64'):
        ops.psf_gram(geom, torch.ones(5, 3, dtype=torch.complex64))
    other = _cpu_geom(P=4)
    other.blvecs = other.blvecs + 1.0
    with pytest.raises(ValueError, match='share blvecs and freqs'):
        ops.psf_gram(geom, w, geom_q=other)
    # everything valid but the device
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ops.psf_gram(geom, w, out=out, rows=good, cols=good, accumulate=True)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ops.psf_gram(geom, w, geom_q=_cpu_geom(P=4))


def test_tile_constants_are_the_kernel_s():
    src = open(kernel_asm.ROOT + '/bayeslim_amd/csrc/psf.hip').read()
    assert '#define RIME_PSF_TILE %d ' % ops.PSF_TILE in src
    assert 'constexpr int PSF_BCHUNK = %d;' % ops.PSF_BCHUNK in src and 'constexpr int PSF_FLUSH = %d;' % ops.PSF_FLUSH in src


def test_psf_kernels_use_no_scratch_and_no_atomics():
    asm, kernels, sizes = kernel_asm.read('psf')
    assert len(kernels) == 2 and len(sizes) == 2 and max(sizes) == 0, (kernels, sizes)
    assert all('psf_gram_kernel' in k for k in kernels) and 'scratch_' not in asm
    assert 'atomic' not in asm and 'v_mfma' not in asm             # one owner per element; vector ALU only
