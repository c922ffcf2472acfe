"""
Host side of the spherical Fourier-Bessel layer (bayeslim_amd/sph_harm.py: sph_bessel_kln, sph_bessel_func, gen_bessel2freq,
SFBModel tables, sfb_binning) against vectors written by the imported reference (tests/golden/make_golden_sfb.py ->
tests/golden/sfb.npz), the in-file oracle of the GPU tests against the same vectors, and the argument checks of
rime_sfb_fwd / rime_sfb_bwd.  No GPU.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import kernel_asm
from conftest import load_golden
from sfb_common import oracle_grad, unpack_basis, relmax


@pytest.fixture(scope='module')
def g():
    return load_golden('sfb')


def shell_kw(g):
    r = g['shell_r']
    return dict(r_min=r.min() - 5, r_max=r.max() + 5, kmax=0.12, dk_factor=0.5)


def test_sph_bessel_kln_shell(g):
    from bayeslim_amd import sph_harm
    keys, kln, _, _ = unpack_basis(g, 'shell')
    for l in keys:
        k = sph_harm.sph_bessel_kln(l, bc_type=2, **shell_kw(g))
        assert k.shape == kln[l].shape, l
        assert np.abs(k / kln[l] - 1).max() < 1e-9, l
    bc1 = np.split(g['shell_kln_bc1'], np.cumsum(g['shell_nk_bc1'])[:-1])
    for l, ref in zip(keys, bc1):
        k = sph_harm.sph_bessel_kln(l, bc_type=1, **shell_kw(g))
        assert k.shape == ref.shape and np.abs(k / ref - 1).max() < 1e-9, l
    # keywords after the roots: every other root; a k = 0 mode for l = 0 only
    assert np.array_equal(sph_harm.sph_bessel_kln(2, decimate=True, **shell_kw(g)), sph_harm.sph_bessel_kln(2, **shell_kw(g))[::2])
    k0 = sph_harm.sph_bessel_kln(0, add_kzero=True, **shell_kw(g))
    assert k0[0] == 0.0 and len(k0) == len(kln[0]) + 1
    assert len(sph_harm.sph_bessel_kln(1, add_kzero=True, **shell_kw(g))) == len(kln[1])
    with pytest.raises(NotImplementedError):
        sph_harm.sph_bessel_kln(1, bc_type=3, **shell_kw(g))
    with pytest.raises(ValueError):
        sph_harm.sph_bessel_kln(1.5, **shell_kw(g))


def test_sph_bessel_kln_ball(g):
    from bayeslim_amd import sph_harm
    keys, kln, _, _ = unpack_basis(g, 'ball')
    for l in keys:
        k = sph_harm.sph_bessel_kln(l, 0.0, 420.0, kmax=0.12, dk_factor=0.5, bc_type=2)
        assert k.shape == kln[l].shape and np.abs(k / kln[l] - 1).max() < 1e-9, l


@pytest.mark.parametrize('tag', ['shell', 'ball'])
def test_gen_bessel2freq_on_the_stored_kln(g, tag):
    from bayeslim_amd import sph_harm
    keys, kln, gln, _ = unpack_basis(g, tag)
    r = g[tag + '_r']
    kw = dict(method='shell', r_crit=r.min()) if tag == 'shell' else dict(method='ball')
    mine, kout = sph_harm.gen_bessel2freq(g[tag + '_l'], r, kbins=kln, dtype=torch.complex128, bc_type=2, renorm=True,
                                          Nproc=4, Ntask=3, use_pathos=True, **kw)            # multiprocessing arguments: ignored
    assert list(mine.keys()) == keys and list(kout.keys()) == keys
    for l in keys:
        assert mine[l].dtype == torch.complex128 and mine[l].shape == gln[l].shape
        assert float(mine[l].imag.abs().max()) == 0.0
        assert relmax(mine[l].real, gln[l]) < 1e-11, l
        assert np.array_equal(kout[l], kln[l])


def test_gen_bessel2freq_computes_its_own_kln(g):
    from bayeslim_amd import sph_harm
    keys, kln, gln, _ = unpack_basis(g, 'shell')
    r = g['shell_r']
    mine, kout = sph_harm.gen_bessel2freq([0, 3, 3], r, dtype=torch.float64, method='shell', bc_type=2, renorm=True,
                                          r_crit=r.min(), **shell_kw(g))
    assert list(mine.keys()) == [0, 3]
    for l in (0, 3):
        assert np.abs(kout[l] / kln[l] - 1).max() < 1e-9
        # the roots agree to 1e-9 relative, k r ~ 1e3 at most: the matrices to ~1e-6
        assert relmax(mine[l], gln[l]) < 1e-5
    with pytest.raises(ValueError):
        sph_harm.sph_bessel_func(0.5, kln[0], r, r_crit=r.min())


def test_sph_bessel_func_renorm(g):
    from bayeslim_amd import sph_harm
    _, kln, _, _ = unpack_basis(g, 'shell')
    r = g['shell_r']
    j = sph_harm.sph_bessel_func(2, kln[2], r, method='shell', r_crit=r.min(), renorm=True, dtype=torch.float64).numpy()
    assert np.allclose(np.sum(r ** 2 * j ** 2, axis=1), np.pi / 2 / kln[2] ** 2, rtol=1e-12)


@pytest.mark.parametrize('tag', ['shell', 'ball'])
def test_sfbmodel_tables(g, tag):
    from bayeslim_amd import sph_harm
    keys, kln, gln, cols = unpack_basis(g, tag)
    sfb = sph_harm.SFBModel()
    sfb.setup_gln(g[tag + '_l'], gln=gln, kln=kln, m=g[tag + '_m'])
    assert list(sfb.params_idx.keys()) == keys
    for l, (a, b), c in zip(keys, g[tag + '_params_idx'], cols):
        assert sfb.params_idx[l] == slice(int(a), int(b))
        idx = sfb.alm_idx[l]
        got = np.arange(sfb.Nlm)[idx] if isinstance(idx, slice) else np.asarray(idx)
        assert np.array_equal(got, c)
        assert sfb.alm_shape[l] == (len(g[tag + '_r']), len(c))
    if tag == 'shell':
        assert sfb.alm_idx[1] == slice(1, 13, 6) and isinstance(sfb.alm_idx[2], list)      # strided; scattered
    assert sfb.Nlmn == int(g[tag + '_Nlmn']) and sfb.Nr == len(g[tag + '_r']) and sfb.Nlm == len(g[tag + '_l'])
    assert np.array_equal(sfb.k_arr, g[tag + '_k_arr'])
    assert np.array_equal(sfb.l_arr, g[tag + '_l_arr'])
    assert np.array_equal(sfb.m_arr, g[tag + '_m_arr'])
    assert sfb.out_dtype == (torch.complex128 if torch.get_default_dtype() == torch.float64 else torch.complex64)


def test_sfbmodel_generates_its_basis(g):
    from bayeslim_amd import sph_harm
    _, kln, gln, _ = unpack_basis(g, 'shell')
    r = g['shell_r']
    sfb = sph_harm.SFBModel()
    sfb.setup_gln(g['shell_l'], r=r, m=g['shell_m'], out_dtype=torch.complex128, method='shell', r_crit=r.min(), **shell_kw(g))
    assert sfb.Nlmn == 335 and sfb.out_dtype == torch.complex128
    assert relmax(sfb.gln[4].real, gln[4]) < 1e-5


def test_sfbmodel_refuses_cpu_tensors_and_complex_bases(g):
    from bayeslim_amd import sph_harm
    keys, kln, gln, _ = unpack_basis(g, 'shell')
    sfb = sph_harm.SFBModel()
    sfb.setup_gln(g['shell_l'], gln=gln, kln=kln)
    with pytest.raises(RuntimeError):
        sfb(torch.zeros(sfb.Nlmn, dtype=torch.complex128))
    with pytest.raises(RuntimeError):
        sfb.forward_gln(torch.zeros(2, sfb.Nlmn))
    bad = {k: v.to(torch.complex128) for k, v in gln.items()}
    bad[3] = bad[3] + 1e-3j
    with pytest.raises(ValueError):
        sph_harm.SFBModel().setup_gln(g['shell_l'], gln=bad, kln=kln)


def test_sfb_binning(g):
    from bayeslim_amd import sph_harm
    p = torch.as_tensor(g['shell_params'])
    var, wg = torch.as_tensor(g['bin_var']), torch.as_tensor(g['bin_wgts'])
    k_arr, l_arr, kb, lb = g['shell_k_arr'], g['shell_l_arr'], g['bin_kbins'], g['bin_lbins']
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)        # the default weights are made in the default dtype
    try:
        cases = [('bin1', {}), ('bin1w', dict(var=var, wgts=wg)), ('bin2', dict(l_arr=l_arr, lbins=lb)),
                 ('bin2w', dict(var=var, wgts=wg, l_arr=l_arr, lbins=lb))]
        for name, kw in cases:
            wg0 = wg.clone()
            out, vout = sph_harm.sfb_binning(p, k_arr, kb, **kw)
            assert out.shape == g[name].shape and out.dtype == torch.complex128
            assert relmax(out, g[name]) < 1e-12, name
            assert relmax(vout, g[name + '_var']) < 1e-12, name
            assert torch.equal(wg, wg0)
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize('case', ['shell', 'shell_real', 'ball'])
def test_in_file_oracle_against_the_reference(g, case):
    tag = 'ball' if case == 'ball' else 'shell'
    keys, _, gln, cols = unpack_basis(g, tag)
    p, w = g[tag + '_params'], g[tag + '_w']
    sfx = ''
    if case == 'shell_real':
        p, w, sfx = p.real.copy(), w.real.copy(), '_real'
    out, gp = oracle_grad(p, w, [gln[k] for k in keys], cols, len(g[tag + '_r']), len(g[tag + '_l']))
    assert out.shape == g[tag + '_out' + sfx].shape
    assert relmax(out, g[tag + '_out' + sfx]) < 1e-11
    assert relmax(gp, g[tag + '_gparams' + sfx]) < 1e-11


def test_sfb_entry_points_reject_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)      # non-null dummy; never dereferenced on a rejected call
    for fn in (lib.rime_sfb_fwd, lib.rime_sfb_bwd):
        #          dtype cplx in   g    blocks cols tiles Nblk Ntile B  Nlmn Nr Nlm out stream
        assert fn(0, 1, one, one, one, one, one, 2, 3, 1, 10, 0, 4, one, None) == -1           # Nr = 0
        assert fn(7, 1, one, one, one, one, one, 2, 3, 1, 10, 5, 4, one, None) == -1           # unknown dtype
        assert fn(0, 1, one, one, None, one, one, 2, 3, 1, 10, 5, 4, one, None) == -1          # Nblk > 0, no block table
        assert fn(0, 1, one, one, one, None, one, 2, 3, 1, 10, 5, 4, one, None) == -1          # Nblk > 0, no column table
        assert fn(0, 1, one, one, one, one, one, 2, -1, 1, 10, 5, 4, one, None) == -1          # Ntile < 0
        assert fn(0, 1, one, one, one, one, None, 2, 3, 1, 10, 5, 4, one, None) == -1          # tiles expected, none given
        assert fn(0, 2, one, one, one, one, one, 2, 3, 1, 10, 5, 4, one, None) == -1           # cplx is 0 or 1
        assert fn(0, 1, None, one, one, one, one, 2, 3, 1, 10, 5, 4, one, None) == -1          # no input
        assert fn(0, 1, one, one, one, one, one, 2, 3, 1, 10, 5, 4, None, None) == -1          # no output
        assert fn(1, 0, one, one, one, one, one, 2, 0, 1, 10, 5, 4, one, None) == 0            # no tile: nothing to do, no launch


def test_sfb_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/sfb.hip: eight kernels (f32 / f64, real / complex, forward / backward), no
    private segment, no matrix-core instruction"""
    asm, kernels, sizes = kernel_asm.read('sfb')
    assert len(kernels) == 8 and all('sfb_kernel' in k for k in kernels), kernels
    assert len(sizes) == 8 and max(sizes) == 0, sizes
    assert not re.findall(r'^\s*scratch_(?:load|store)', asm, flags=re.M)
    assert 'v_mfma' not in asm
