"""
Host side of the filter layer (bayeslim_amd/filt.py, ops.filt_tables / filt_tiles / filt_pack) against vectors written by the
imported reference (tests/golden/make_golden_filt.py -> tests/golden/filt.npz), the CPU oracle of the GPU tests against the
same vectors, the tile-list and table properties the kernel relies on, the argument checks of rime_filt_apply and the
no-scratch property of its gfx950 assembly.  No GPU.
"""
import copy
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

import kernel_asm
from filt_common import golden, oracle_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def g():
    return golden()


def close(a, ref, tol):
    """max |a - ref| relative to the largest element of the stored array"""
    a = torch.as_tensor(a)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).abs().max() / ref.abs().max()) < tol


def test_covariance_builders(g):
    from bayeslim_amd import filt
    x, x2 = g['bx'], g['bx2']
    assert close(filt.rbf_cov(x, 0.3, amp=2.0), g['rbf'], 1e-10)
    assert close(filt.rbf_cov(x, 0.3, x2=x2), g['rbf_x2'], 1e-10)
    assert close(filt.exp_cov(x, 0.4, amp=1.5), g['exp'], 1e-10)
    assert close(filt.exp_cov(x, 0.4, x2=x2), g['exp_x2'], 1e-10)
    assert close(filt.sinc_cov(x, 0.25), g['sinc'], 1e-10)
    assert close(filt.sinc_cov(x, 0.25, x2=x2), g['sinc_x2'], 1e-10)
    assert close(filt.phasor_mat(x, 1.7), g['phasor'], 1e-10)
    assert close(filt.phasor_mat(x, 1.7, neg=False, x2=x2), g['phasor_pos_x2'], 1e-10)
    assert close(filt.gauss_sinc_cov(x, 0.5, 0.3), g['gauss_sinc'], 1e-10)
    assert close(filt.gauss_sinc_cov(x, 0.5, 0.3, x2=x2), g['gauss_sinc_x2'], 1e-10)
    assert filt.rbf_cov(x, 0.3, dtype=torch.float32).dtype == torch.float32


def test_gen_cov_modes(g):
    from bayeslim_amd import filt
    A, ev = filt.gen_cov_modes(g['rbf'], N=4)
    assert close(ev, g['modes_evals'], 1e-10)
    # eigenvectors up to sign
    sgn = torch.sign((A * g['modes_N4']).sum(0))
    assert close(A * sgn, g['modes_N4'], 1e-8)
    A, _ = filt.gen_cov_modes(g['rbf'], rcond=1e-6)
    assert A.shape == g['modes_rcond'].shape
    with pytest.raises(AssertionError):
        filt.gen_cov_modes(g['rbf'], N=2, rcond=1e-3)


def test_invert_matrix_and_gpfilter(g):
    from bayeslim_amd import filt
    C = g['inv_C']
    for inv, kw in (('inv', {}), ('diag', {}), ('pinv', dict(rcond=1e-8, hermitian=True)), ('chol', dict(eps=1e-2))):
        assert close(filt.invert_matrix(C.clone(), inv=inv, **kw), g['inv_' + inv], 1e-10), inv
    assert torch.equal(filt.invert_matrix(torch.tensor([2.0, 4.0])), torch.tensor([0.5, 0.25]))
    with pytest.raises(NameError):
        filt.invert_matrix(C.clone(), inv='nope')
    for inv in ('pinv', 'chol'):
        gp = filt.GPFilter(g['gp_Cs'].clone(), g['gp_Cn'].clone(), inv=inv, rcond=1e-12)
        assert close(gp.G, g['gp_G_' + inv], 1e-10) and close(gp.V, g['gp_V_' + inv], 1e-10), inv
    # setup_filter with new covariances rebuilds G (the reference's MatFilter.setup_filter raises NameError instead)
    gp.setup_filter(Cn=g['gp_Cn'] * 2)
    assert not close(gp.G, g['gp_G_chol'], 1e-10)
    m = filt.MatFilter(g['mat_G_real'])
    m.setup_filter(g['rect_G'])
    assert m.G.shape == g['rect_G'].shape


CASES = [('mat_real_res0', 'mat_x', 'mat_G_real', False, None), ('mat_real_res1', 'mat_x', 'mat_G_real', True, None),
         ('mat_cplx_res0', 'mat_x', 'mat_G_cplx', False, None), ('mat_cplx_res1', 'mat_x', 'mat_G_cplx', True, None),
         ('rect', 'mat_x', 'rect_G', False, None), ('inp_res0', 'mat_x', 'inp_G', False, 'inp_idx'),
         ('inp_res1', 'mat_x', 'inp_G', True, 'inp_idx')]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_oracle_against_the_reference(g, case):
    tag, xk, Gk, res, ik = case
    y, _, gx, _ = oracle_filter(g[xk], g[Gk], residual=res, input_idx=None if ik is None else g[ik])
    assert close(y, g[tag + '_out'], 1e-12)
    assert close(2 * gx, g[tag + '_grad'], 1e-12)


def wedge_b2f(g):
    from bayeslim_amd import filt
    bls = [tuple(b) for b in g['wedge_bls'].tolist()]
    f2b = {0: [tuple(b) for b in g['wedge_bls0'].tolist()], 1: [tuple(b) for b in g['wedge_bls1'].tolist()]}
    w = filt.WedgeFilter([filt.MatFilter(g['mat_G_real'], residual=True), filt.MatFilter(g['mat_G_cplx'], residual=True)], f2b, bls=bls)
    return w, bls, f2b


def test_oracle_against_the_reference_wedge_and_dim(g):
    w, bls, _ = wedge_b2f(g)
    b2f = w._bl2filt(bls)
    assert b2f == (0, -1, 1, 0, -1, 1, 0)
    G = torch.stack([g['mat_G_real'].to(torch.complex128), g['mat_G_cplx']])
    y, _, gx, _ = oracle_filter(g['wedge_x'], G, residual=True, bl2filt=b2f)
    assert close(y, g['wedge_out'], 1e-12) and close(y, g['wedge_out_vd'], 1e-12)
    assert close(2 * gx, g['wedge_grad'], 1e-12)
    y, _, gx, _ = oracle_filter(g['dim2_x'].movedim(-2, -1), g['mat_G_cplx'], residual=True)
    assert close(y.movedim(-1, -2), g['dim2_out'], 1e-12) and close(2 * gx.movedim(-1, -2), g['dim2_grad'], 1e-12)


@pytest.mark.parametrize('layout', [(1, 1, 1, (0,)), (1, 30, 5, (0,) * 30), (4, 9, 5, (2, -1, 0, 1, 1, -1, 0, 2, 2)),
                                    (2, 3, 70, (1, 1, -1))])
def test_tile_list_properties(layout):
    from bayeslim_amd import ops
    outer, Nbl, inner, b2f = layout
    tiles, npass = ops.filt_tiles(outer, Nbl, inner, b2f)
    again, _ = ops.filt_tiles(outer, Nbl, inner, b2f)
    assert tiles.dtype == np.int32 and tiles.shape[1] == 1 + ops.FILT_TILE_LINES and np.array_equal(tiles, again)
    fl = np.broadcast_to(np.asarray(b2f)[None, :, None], (outer, Nbl, inner)).reshape(-1)
    lines = tiles[:, 1:]
    listed = lines[lines >= 0]
    assert np.array_equal(np.sort(listed), np.arange(outer * Nbl * inner))           # every line in exactly one tile
    for t in tiles:
        valid = t[1:][t[1:] >= 0]
        assert len(valid) and (fl[valid] == t[0]).all()                              # ... of its own filter
        assert (t[1:][:len(valid)] >= 0).all()                                       # padding at the end of the tile only
    for f in np.unique(tiles[:, 0]):
        own = tiles[tiles[:, 0] == f][:, 1:]
        assert (own[:-1] >= 0).all()                                                 # ... and in a filter's last tile only
        flat = own[own >= 0]
        assert (np.diff(flat) > 0).all()
    assert npass == (tiles[:, 0] < 0).sum() and (np.diff(np.where(tiles[:, 0] < 0, 1 << 30, tiles[:, 0])) >= 0).all()
    nopass, n0 = ops.filt_tiles(outer, Nbl, inner, b2f, with_pass=False)
    assert n0 == 0 and np.array_equal(nopass, tiles[tiles[:, 0] >= 0])
    with pytest.raises(ValueError):
        ops.filt_tiles(outer, Nbl + 1, inner, b2f)


def test_tables_of_the_three_modes():
    from bayeslim_amd import ops
    M, K = 3, 6
    eyeK, eyeM = np.arange(K), np.arange(M)
    t = ops.filt_tables(M, K)                                             # y = G x; gx = G^H g
    assert t['Ny'] == M and np.array_equal(t['fwd'][0], eyeK) and np.array_equal(t['fwd'][1], eyeM)
    assert not t['fwd'][2].any() and t['fwd'][3] == 1.0
    assert np.array_equal(t['bwd'][0], eyeM) and np.array_equal(t['bwd'][1], eyeK) and not t['bwd'][2].any() and t['bwd'][3] == 1.0
    t = ops.filt_tables(K, K, residual=True)                              # y = x - G x; gx = g - G^H g
    assert t['fwd'][2].all() and t['fwd'][3] == -1.0 and t['bwd'][2].all() and t['bwd'][3] == -1.0
    idx = [1, 4, 5]
    for form in (idx, torch.as_tensor(idx), np.isin(eyeK, idx), [1, -2, -1]):
        t = ops.filt_tables(M, K, input_idx=form)                         # y[idx] = G x; gx = G^H g[idx] + (j not in idx) g
        assert t['Ny'] == K and np.array_equal(t['fwd'][1], idx) and np.array_equal(t['bwd'][0], idx)
        assert np.array_equal(t['bwd'][1], eyeK) and np.array_equal(t['bwd'][2], [1, 0, 1, 1, 0, 0]) and not t['fwd'][2].any()
    t = ops.filt_tables(M, K, residual=True, input_idx=idx)               # y[idx] = x[idx] - G x; gx = g - G^H g[idx]
    assert t['fwd'][2].all() and t['bwd'][2].all() and t['bwd'][3] == -1.0
    for d in ('fwd', 'bwd'):
        assert t[d][0].dtype == np.int32 and t[d][1].dtype == np.int32
    with pytest.raises(ValueError):
        ops.filt_tables(M, K, residual=True)                              # residual of a rectangular filter
    with pytest.raises(ValueError):
        ops.filt_tables(M, K, input_idx=[1, 1, 2])
    with pytest.raises(ValueError):
        ops.filt_tables(M, K, input_idx=[1, 2])
    with pytest.raises(ValueError):
        ops.filt_tables(M, K, input_idx=[1, 2, 6])


def test_pack_of_real_and_complex_filters():
    from bayeslim_amd import ops
    rng = np.random.default_rng(5)
    W = torch.as_tensor(rng.normal(size=(2, 3, 4)) + 1j * rng.normal(size=(2, 3, 4)))
    p = ops.filt_pack(W)
    assert p.shape == (2, 8, 3) and p.is_contiguous() and not p.is_complex()
    assert torch.equal(p[:, 0::2], W.real.transpose(1, 2)) and torch.equal(p[:, 1::2], -W.imag.transpose(1, 2))
    assert torch.equal(ops.filt_pack(W.real), W.real.transpose(1, 2))
    with pytest.raises(ValueError):
        ops.filt_pack(W[0])


def test_bad_arguments_are_rejected_without_launching():
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)          # non-null dummy; never dereferenced on a rejected call

    def call(dtype=0, wcplx=0, x=one, W=one, ic=one, oc=one, base=one, tiles=one, Ntile=1, Npass=0, Nfilt=1, M=4, K=4, Nx=4,
             Ny=4, Nlines=10, s=1.0, y=one):
        return lib.rime_filt_apply(dtype, wcplx, x, W, ic, oc, base, tiles, Ntile, Npass, Nfilt, M, K, Nx, Ny, Nlines, s, y, None)

    assert call(dtype=7) == -1 and call(wcplx=2) == -1
    assert call(M=0) == -1 and call(K=0) == -1 and call(K=-3) == -1 and call(Nfilt=0) == -1
    assert call(ic=None) == -1 and call(oc=None) == -1 and call(base=None) == -1 and call(tiles=None) == -1
    assert call(x=None) == -1 and call(W=None) == -1 and call(y=None) == -1
    assert call(Npass=1, Nx=4, Ny=5) == -1                   # a copied line keeps its length
    assert call(Npass=2, Ntile=1) == -1 and call(s=0.5) == -1 and call(Nlines=-1) == -1 and call(Nlines=1 << 31) == -1
    assert call(Ntile=0) == 0 and call(Nlines=0) == 0        # nothing to do: no launch either


def test_filt_assembly_uses_no_scratch():
    asm, kernels, sizes = kernel_asm.read('filt')
    assert len(kernels) == 4 and all('filt_kernel' in k for k in kernels), kernels       # {f32, f64} x {real, complex W}
    assert not re.findall(r'^\s*scratch_(?:load|store)', asm, flags=re.M)
    assert len(sizes) == 4 and max(sizes) == 0, sizes
    lds = [int(x) for x in re.findall(r'\.amdhsa_group_segment_fixed_size (\d+)', asm)]
    assert max(lds) < 160 * 1024, lds
    assert len(re.findall(r'v_mfma_f32_32x32x2_f32', asm)) >= 2                           # float32 runs on the f32-input MFMA
    rec = open(os.path.join(ROOT, 'bayeslim_amd', 'lib', 'obj', 'filt.scan')).read()
    assert rec.startswith('no packed-f32 reader'), rec


def test_objects_pickle_and_deepcopy_without_a_plan(g):
    from bayeslim_amd import filt
    w, bls, f2b = wedge_b2f(g)
    gp = filt.GPFilter(g['gp_Cs'].clone(), g['gp_Cn'].clone(), residual=True, input_idx=None)
    ls = filt.LstSqFilter(g['mat_G_real'])
    assert ls.residual is True
    for obj in (w, gp, ls, w.filters[1]):
        obj.__dict__['_plans'] = {'stale': object()}
        for cp in (pickle.loads(pickle.dumps(obj)), copy.deepcopy(obj)):
            assert '_plans' not in cp.__dict__ and type(cp) is type(obj)
    cp = copy.deepcopy(w)
    assert torch.equal(cp.filters[1].G, w.filters[1].G) and cp.filters[1].G is not w.filters[1].G and cp.filt2bls == f2b
    gp.push(torch.float32)
    assert gp.G.dtype == torch.float32 and '_plans' not in gp.__dict__
    w.filters[1].push(torch.complex64)
    assert w.filters[1].G.dtype == torch.complex64


def test_wedge_member_mismatch_is_named(g):
    from bayeslim_amd import filt
    G = g['mat_G_real']
    mk = lambda *f: filt.WedgeFilter(list(f), {0: [(0, 1)], 1: [(0, 2)]}, bls=[(0, 1), (0, 2)])
    with pytest.raises(ValueError, match='residual'):
        mk(filt.MatFilter(G, residual=True), filt.MatFilter(G))._members()
    with pytest.raises(ValueError, match='shape of G'):
        mk(filt.MatFilter(G), filt.MatFilter(g['rect_G']))._members()
    with pytest.raises(ValueError, match='input_idx'):
        mk(filt.MatFilter(g['inp_G'], input_idx=g['inp_idx']), filt.MatFilter(g['inp_G'], input_idx=g['inp_idx'] - 1))._members()
    with pytest.raises(ValueError, match='dim'):
        mk(filt.MatFilter(G, dim=-2), filt.MatFilter(G, dim=-2))._members()
    with pytest.raises(ValueError, match='belongs to the groups'):
        filt.WedgeFilter([filt.MatFilter(G), filt.MatFilter(G)], {0: [(0, 1)], 1: [(0, 1)]}, bls=[(0, 1)])._bl2filt([(0, 1)])


def test_no_cpu_path_and_no_gradient_for_G(g):
    from bayeslim_amd import filt, ops
    with pytest.raises(RuntimeError, match='GPU'):
        filt.MatFilter(g['mat_G_real'])(g['mat_x'])
    with pytest.raises(ValueError, match='requires grad'):
        ops.FiltPlan(g['mat_G_real'].clone().requires_grad_(True))
