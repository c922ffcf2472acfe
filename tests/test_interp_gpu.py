"""
GPU checks of csrc/interp.hip (ops.interp_gather and ops.beam_sky_product with their adjoints) against the float64
restatement of tests/interp_common.py, case tables from there (tests/test_interp_host.py shows which branch each reaches).
Every comparison is elementwise at the derived bound (n + 4) u S of interp_common or exact; every case is run twice and
must give the same bits, forward and backward.
"""
import numpy as np
import pytest
import torch

import interp_common as ic

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from bayeslim_amd import ops as _ops
    return _ops


def draw(rng, shape, cplx, prec):
    """normal draws rounded to the working precision: the restatement sees what the kernel sees"""
    x = rng.normal(size=shape)
    return (x + 1j * rng.normal(size=shape)).astype(ic.CDT[prec]) if cplx else x.astype(ic.RDT[prec])


def dev(x):
    return torch.as_tensor(x).to(DEV)


def close(got, ref, S, n, prec, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape, what
    if np.iscomplexobj(ref):
        close(got.real, ref.real, S.real, n, prec, what + ' (real part)')
        close(got.imag, ref.imag, S.imag, n, prec, what + ' (imaginary part)')
        return
    assert np.isfinite(got).all(), what
    excess = np.abs(got.astype(np.float64) - ref) / ic.bound(S, n, prec)
    print('%s: worst error / bound %.3f' % (what, excess.max()))
    assert excess.max() <= 1.0, what


def stencil_on_gpu(ops, inds, w, Npb, prec):
    return ops.InterpStencil(dev(inds), dev(w.astype(ic.RDT[prec])), Npb)


def gather_twice(ops, m, st, gout, out_stride=None):
    """forward and adjoint of ops.interp_gather for the cotangent gout, run twice: equal bits"""
    res = []
    for _ in range(2):
        x = dev(m).requires_grad_(True)
        y = ops.interp_gather(x, st, out_stride=out_stride)
        gm, = torch.autograd.grad(y, x, dev(gout))
        res.append((y.detach(), gm))
    # (bitwise: NaN-free by the checks that follow)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    return res[0]


def check_gather(ops, m, inds, w, Npb, gout, prec, stride, what):
    """forward and adjoint against the restatement; `stride` > P: padding columns exactly 0, and their cotangent (NaN) unread"""
    P = inds.shape[0]
    w = w.astype(ic.RDT[prec])
    st = stencil_on_gpu(ops, inds, w, Npb, prec)
    assert (st.csr_ptr.diff().cpu().numpy() == ic.csr_lengths(inds, w, Npb)).all()
    gpad = np.full(gout.shape[:-1] + (stride,), np.nan, dtype=gout.dtype)
    gpad[..., :P] = gout
    y, gm = gather_twice(ops, m, st, gpad, out_stride=stride)
    assert y.shape == m.shape[:-1] + (stride,) and gm.shape == m.shape and y.dtype == gm.dtype == dev(m).dtype
    assert (y[..., P:] == 0).all()
    ref, S, n = ic.gather(m, inds, w)
    close(y[..., :P], ref, S, n, prec, what + ' forward')
    ref, S, n = ic.gather_adjoint(gout, inds, w, Npb)
    close(gm, ref, S, n, prec, what + ' adjoint')
    return y, gm


# --------------------------------------------------------------------------------------------- 1. widths
@pytest.mark.parametrize('Nnn,cplx,prec,R,P,padded', ic.GATHER_CASES)
def test_gather_and_adjoint_across_widths(ops, Nnn, cplx, prec, R, P, padded):
    Npb = ic.GATHER_NPB
    inds, w, _ = ic.make_stencil(ic.stencil_seed(1, Nnn, R, P), Npb, P, Nnn)
    rng = np.random.default_rng(ic.stencil_seed(11, Nnn, R, P))
    m, gout = draw(rng, (R, Npb), cplx, prec), draw(rng, (R, P), cplx, prec)
    check_gather(ops, m, inds, w, Npb, gout, prec, ops.pad_to_tile(P) if padded else P, 'gather Nnn=%d' % Nnn)


# --------------------------------------------------------------------------------------------- 2. weight 0
@pytest.mark.parametrize('Nnn,cplx,prec', ic.POISON_CASES)
def test_weight_zero_keeps_non_finite_entries_out(ops, Nnn, cplx, prec):
    """a slot of weight 0 that names a node where the map holds NaN / +inf adds nothing to the forward, and a NaN / inf
    cotangent at a point whose weights are all 0 nothing to the map gradient (the inverse index leaves such entries out, so
    forward and adjoint stay adjoint to each other)"""
    Npb, R, P = ic.GATHER_NPB, ic.POISON_R, ic.POISON_P
    inds, w, planted = ic.make_stencil(ic.stencil_seed(2, Nnn), Npb, P, Nnn, dead_points=2)
    bad = planted[0]                                                  # the node of the empty list: only weight-0 slots name it
    e = np.flatnonzero(w.reshape(-1) == 0)
    inds.reshape(-1)[e[::3]] = bad
    assert (inds == bad).sum() >= 3 and (w[inds == bad] == 0).all()
    rng = np.random.default_rng(ic.stencil_seed(12, Nnn))
    m, gout = draw(rng, (R, Npb), cplx, prec), draw(rng, (R, P), cplx, prec)
    both = (lambda v: complex(v, v)) if cplx else (lambda v: v)        # real and imaginary part alike
    m[0::2, bad], m[1::2, bad] = both(np.nan), both(np.inf)
    gout[:, planted['dead'][0]], gout[:, planted['dead'][1]] = both(np.nan), both(np.inf)
    y, gm = check_gather(ops, m, inds, w, Npb, gout, prec, P, 'poisoned Nnn=%d' % Nnn)
    assert torch.isfinite(torch.view_as_real(y) if cplx else y).all()
    assert (gm[:, bad] == 0).all()


@pytest.mark.parametrize('Nnn', [1, 4])
@pytest.mark.parametrize('cplx,prec', [(False, 'f32'), (True, 'f64')])
def test_all_zero_stencil_gives_exact_zeros(ops, Nnn, cplx, prec):
    """Nnn = 1: the row-major adjoint on an empty inverse index; Nnn = 4: the early return of the autograd function"""
    Npb, R, P = ic.GATHER_NPB, ic.POISON_R, ic.POISON_P
    inds, w, _ = ic.make_stencil(ic.stencil_seed(2, Nnn), Npb, P, Nnn, all_zero=True)
    rng = np.random.default_rng(Nnn)
    m, gout = draw(rng, (R, Npb), cplx, prec), draw(rng, (R, P), cplx, prec)
    m[:, 5], gout[:, 7] = np.nan, np.inf
    st = stencil_on_gpu(ops, inds, w, Npb, prec)
    assert st.csr_src.numel() == 0
    y, gm = gather_twice(ops, m, st, gout)
    assert y.shape == (R, P) and gm.shape == (R, Npb)
    assert (y == 0).all() and (gm == 0).all()


# --------------------------------------------------------------------------------------------- 3. CSR scatter
@pytest.mark.parametrize('Nnn,R,cplx,prec', ic.SCATTER_CASES)
def test_csr_scatter_rows_and_list_lengths(ops, Nnn, R, cplx, prec):
    Npb, P = ic.SCATTER_NPB, ic.SCATTER_P
    inds, w, _ = ic.make_stencil(ic.stencil_seed(3, Nnn), Npb, P, Nnn)
    rng = np.random.default_rng(ic.stencil_seed(13, Nnn, R))
    m, gout = draw(rng, (R, Npb), cplx, prec), draw(rng, (R, P), cplx, prec)
    check_gather(ops, m, inds, w, Npb, gout, prec, P, 'CSR scatter Nnn=%d RN=%d' % (Nnn, R * (2 if cplx else 1)))


# --------------------------------------------------------------------------------------------- 4. row-major scatter
@pytest.mark.parametrize('R,cplx,prec,Npb,extra', ic.ROWS_CASES)
def test_row_major_scatter_of_the_one_node_stencil(ops, R, cplx, prec, Npb, extra):
    P = ic.ROWS_P
    inds, w, _ = ic.make_stencil(ic.stencil_seed(4, R, Npb), Npb, P, 1)
    rng = np.random.default_rng(ic.stencil_seed(14, R, Npb))
    m, gout = draw(rng, (R, Npb), cplx, prec), draw(rng, (R, P), cplx, prec)
    check_gather(ops, m, inds, w, Npb, gout, prec, P + extra, 'row-major scatter R=%d' % R)


# --------------------------------------------------------------------------------------------- 5. rows beyond one grid
@pytest.fixture(scope='module')
def big_inputs():
    rng = np.random.default_rng(5)
    R, Npb, P = ic.BIG_R, ic.BIG_NPB, ic.BIG_P
    m = (rng.standard_normal((R, Npb), dtype=np.float32) + 1j * rng.standard_normal((R, Npb), dtype=np.float32)).astype(np.complex64)
    g = (rng.standard_normal((R, P), dtype=np.float32) + 1j * rng.standard_normal((R, P), dtype=np.float32)).astype(np.complex64)
    return m, g


def _big_rows():
    """the first and the last 16 rows, the rows either side of the end of the first launch, a strided sample between"""
    R, edge = ic.BIG_R, ic.GRID_Y * ic.RT
    return np.unique(np.concatenate([np.arange(16), np.arange(R - 16, R), np.arange(edge - 16, edge + 9), np.arange(0, R, 4099)]))


@pytest.mark.parametrize('Nnn', [1, 4])
def test_rows_beyond_one_grid(ops, big_inputs, Nnn):
    """R = 65535 * 8 + 9 map rows: the forward (and for Nnn = 1 the row-major adjoint behind it) needs a second launch.  The
    sampled rows are compared at the bound; every row outside the sample must be written (the output starts as NaN-free
    zeros, a skipped row of normal draws would be exactly 0 in all its columns)"""
    m, g = big_inputs
    R, Npb, P = ic.BIG_R, ic.BIG_NPB, ic.BIG_P
    rng = np.random.default_rng(50 + Nnn)
    inds = rng.integers(0, Npb, (P, Nnn))
    w = rng.uniform(0.25, 1.0, (P, Nnn)).astype(np.float32)
    w[2, 0] = 0.0
    inds[0, 0], inds[1, 0] = 1, 1                                      # a node selected twice, by live weights
    st = stencil_on_gpu(ops, inds, w, Npb, 'f32')
    rows = _big_rows()
    ref, S, n = ic.gather(m[rows], inds, w)
    x = dev(m).requires_grad_(Nnn == 1)
    y = ops.interp_gather(x, st)
    assert y.shape == (R, P)
    close(y.detach()[dev(rows)], ref, S, n, 'f32', 'big forward Nnn=%d' % Nnn)
    live = torch.as_tensor((w != 0).any(1)).to(DEV)
    assert (y.detach()[:, live] != 0).all()                           # no row left out
    y2 = ops.interp_gather(dev(m), st)
    assert torch.equal(y.detach(), y2)
    if Nnn > 1:
        return                                                        # the CSR adjoint's row limit is its own
    gm, = torch.autograd.grad(y, x, dev(g))
    ref, S, n = ic.gather_adjoint(g[rows], inds, w, Npb)
    close(gm[dev(rows)], ref, S, n, 'f32', 'big adjoint')
    sel = torch.as_tensor(ic.csr_lengths(inds, w, Npb) > 0).to(DEV)
    assert (gm[:, sel] != 0).all() and (gm[:, ~sel] == 0).all()
    y3 = ops.interp_gather(x, st)
    gm2, = torch.autograd.grad(y3, x, dev(g))
    assert torch.equal(gm, gm2)


# --------------------------------------------------------------------------------------------- 6. psky builder
def psky_twice(ops, bmap, sky, st, cut, pos, Nt, Ps, g):
    res = []
    for _ in range(2):
        b, s = dev(bmap).requires_grad_(True), dev(sky).requires_grad_(True)
        out = ops.beam_sky_product(b, s, st, cut, pos, Nt, Ps)
        gb, gs = torch.autograd.grad(out, (b, s), dev(g))
        res.append((out.detach(), gb, gs))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    return res[0]


@pytest.mark.parametrize('Nnn,prec,R,Nt', ic.PSKY_CASES)
def test_psky_builder_instantiations(ops, Nnn, prec, R, Nt):
    Npb, Npix, Ps = ic.PSKY_NPB, ic.PSKY_NPIX, ic.PSKY_PS
    Q = Nt * Ps
    # the case runs the time split it names: the library asks for S planes of workspace, or for none
    S, Tc = ic.sky_grad_splits(R, Npix, Nt)
    code = ops.RIME_F32 if prec == 'f32' else ops.RIME_F64
    nws = int(ops.lib.rime_beam_sky_bwd_workspace(code, R, Npix, Nt))
    assert nws == (S * R * Npix * (4 if prec == 'f32' else 8) if S > 1 else 0)
    assert (S > 1) == (Nt >= 5)

    inds, w, _ = ic.make_stencil(ic.stencil_seed(6, Nnn, Nt), Npb, Q, Nnn)
    w = w.astype(ic.RDT[prec])
    cut, pos = ic.make_cut(ic.stencil_seed(16, Nt), Nt, Ps, Npix)
    rng = np.random.default_rng(ic.stencil_seed(26, Nnn, R, Nt))
    bmap, sky, g = draw(rng, (R, Npb), False, prec), draw(rng, (R, Npix), False, prec), draw(rng, (R, Q), False, prec)
    st = stencil_on_gpu(ops, inds, w, Npb, prec)
    out, gb, gs = psky_twice(ops, bmap, sky, st, dev(cut.astype(np.int32)), dev(pos.astype(np.int32)), Nt, Ps, g)
    what = 'psky Nnn=%d R=%d Nt=%d %s' % (Nnn, R, Nt, prec)
    ref, Sa, n = ic.beam_sky(bmap, sky, inds, w, cut)
    close(out, ref, Sa, n, prec, what + ' forward')
    assert (out[:, dev(cut == Npix)] == 0).all()                       # padded points
    ref, Sa, n = ic.beam_sky_grad_map(g, sky, inds, w, cut, Npb)
    close(gb, ref, Sa, n, prec, what + ' map gradient')
    ref, Sa, n = ic.beam_sky_grad_sky(g, bmap, inds, w, cut, Npix)
    close(gs, ref, Sa, n, prec, what + ' sky gradient')
    unseen = (pos >= 0).sum(0) == 0
    assert unseen[ic.NEVER] and (gs[:, dev(unseen)] == 0).all()
