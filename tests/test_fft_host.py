"""
CPU-side checks of the Fourier layer (bayeslim_amd/fft.py, ops.FFTPlan, rime_fft_apply): windows, the float64 oracle of
tests/fft_common.py and the averaging of dataset.py against the reference's recorded results (tests/golden/fft.npz), the
host plan (radix lists, twiddle tables), argument validation without a GPU, pickling, and that the accuracy bound the GPU
tests assert is one the reference's own float32 transform meets.
"""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

import fft_common as fc
import kernel_asm


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


@pytest.mark.parametrize('name', fc.WINDOWS)
def test_gen_window_against_the_reference(f64, name):
    from bayeslim_amd import fft
    g = fc.golden()
    kw = fc.WINDOW_KW.get(name, {})
    for N in (16, 9):
        w = fft.gen_window(name, N, **kw)
        assert w.dtype == torch.float64 and w.shape == (N,)
        assert float((w - g['win_%s_%d' % (name, N)]).abs().max()) <= 1e-12, (name, N)
    w = fft.gen_window(name, 16, edgecut=(2, 3), **kw)
    assert float((w - g['win_%s_ec' % name]).abs().max()) <= 1e-12
    assert float(w[:2].abs().max()) == 0.0 and float(w[-3:].abs().max()) == 0.0


def test_gen_window_aliases_default_dtype_and_unknown_names():
    from bayeslim_amd import fft
    assert fft.gen_window('bh', 8).dtype == torch.get_default_dtype()
    for a, b in (('bh', 'blackmanharris'), ('bh4', 'blackman-harris'), ('hann', 'hanning'), (None, 'tophat'),
                 ('bh7', 'blackmanharris-7term'), ('cs9', 'cosinesum-9term'), ('cs11', 'cosinesum-11term')):
        assert torch.equal(fft.gen_window(a, 11), fft.gen_window(b, 11))
    assert torch.equal(fft.gen_window('hann', 1), torch.ones(1))
    with pytest.raises(ValueError):
        fft.gen_window('no_such_window', 8)
    with pytest.raises(ValueError):
        fft.gen_window('gaussian', 8)


@pytest.mark.parametrize('case', range(len(fc.FWD_CASES)))
def test_oracle_against_the_reference(f64, case):
    """the float64 oracle of fft_common (what the GPU tests compare with) on the reference's recorded FFT.forward outputs"""
    from bayeslim_amd import fft
    g = fc.golden()
    kw, dim = fc.FWD_CASES[case]
    kw = dict(kw)
    x = g['fwd_x'] if dim in (-1, 2) else g['fwd_x'].movedim(-1, dim).contiguous()
    F = fft.FFT(dim=dim, N=12, ndim=3, dx=0.5, **kw)               # the window and the flags as the product builds them
    y = fc.oracle(x, dim=dim, ifft=F.ifft, win=F.win, fftshift=F.fftshift, norm=F.norm, abs=F.abs, peaknorm=F.peaknorm,
                  square=F.square)
    ref = g['fwd_%d' % case]
    assert y.shape == ref.shape and y.dtype == ref.dtype
    assert float((y - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max()))


def test_oracle_peak_and_adjoint(f64):
    from bayeslim_amd import fft
    g = fc.golden()
    for i, kw in enumerate(fc.PEAK_CASES):
        F = fft.PeakDelay(dim=2, N=32, ndim=3, dx=0.25, **kw)
        y = fc.oracle(g['peak_x'], dim=2, ifft=F.ifft, win=F.win, fftshift=F.fftshift, norm=F.norm, abs=F.abs,
                      peaknorm=F.peaknorm, square=F.square)
        pk = fc.oracle_peak(y, float(F.start), float(F.df))
        ref = g['peak_%d' % i][..., 0]
        assert float((pk - ref).abs().max()) <= 1e-12 * float(F.df) * 32, i
    # the plain case finds the tones: bins 3.3, 9.71, ... of 32 at df = 1 / (32 * 0.25), to the estimator's accuracy
    F = fft.PeakDelay(dim=2, N=32, ndim=3, dx=0.25)
    tones = g['peak_tones'].reshape(2, 3)
    want = torch.where(tones >= 16, tones - 32, tones) * float(F.df)
    assert float((g['peak_0'][..., 0] - want).abs().max()) < 0.05 * float(F.df)
    # adjoint of the linear part against autograd
    rng = np.random.default_rng(5)
    for N, ifft, shift, norm in ((7, False, True, None), (8, True, True, 'ortho'), (9, True, False, 'forward'), (6, False, False, None)):
        x = fc.tone_input(rng, (3, N)).requires_grad_(True)
        w, c = fc.window_vec(rng, N), fc.tone_input(rng, (3, N))
        xw = x * w
        y = torch.fft.ifft(torch.fft.ifftshift(xw, dim=-1) if shift else xw, norm=norm) if ifft else torch.fft.fft(xw, norm=norm)
        y = torch.fft.fftshift(y, dim=-1) if (shift and not ifft) else y
        assert torch.equal(y.detach(), fc.oracle_linear(x, ifft=ifft, win=w, fftshift=shift, norm=norm))
        gx, = torch.autograd.grad(y, x, c)
        mine = fc.oracle_adjoint(c, ifft=ifft, win=w, fftshift=shift, norm=norm)
        assert float((gx - mine).abs().max()) < 1e-12 * float(gx.abs().max())


def test_fft_object_attributes(f64):
    from bayeslim_amd import fft
    F = fft.FFT(dim=4, ndim=5, N=12, dx=0.5, window='bh', edgecut=2)
    assert torch.equal(F.freqs, torch.fft.fftshift(torch.fft.fftfreq(12, d=0.5)))
    assert float(F.start) == float(F.freqs[0]) and abs(float(F.df) - 1 / 6.0) < 1e-15
    assert F.edgecut == (2, 2) and tuple(F.win.shape) == (1, 1, 1, 1, 12)
    assert float(F.win.reshape(-1)[:2].abs().max()) == 0 and float(F.win.reshape(-1)[2]) > 0
    F = fft.FFT(dim=0, N=5, fftshift=False)
    assert torch.equal(F.freqs, torch.fft.fftfreq(5, d=1.0)) and F.win is None and F.edgecut == (0, 0)
    F = fft.FFT()
    assert F.freqs is None and F.df is None and F.dx is None and F.start == 0.0
    with pytest.raises(ValueError, match='needs N'):
        fft.PeakDelay(dim=0)(torch.zeros(4, dtype=torch.complex64))
    with pytest.raises(RuntimeError):
        fft.FFT(dim=0)(torch.zeros(4, dtype=torch.complex64))            # a CPU tensor: no CPU path
    with pytest.raises(RuntimeError):
        fft.FFT(dim=0)(np.zeros(4, dtype=np.complex64))


def test_fft_pickles_and_deepcopies(f64):
    from bayeslim_amd import fft, ops
    F = fft.PeakDelay(dim=1, ndim=2, N=16, dx=2.0, window='hann', abs=True)
    F.__dict__['_plans'] = {'k': ops.FFTPlan(16, torch.float32, 'cuda')}       # as after a first call (tables not built)
    for G in (pickle.loads(pickle.dumps(F)), copy.deepcopy(F)):
        assert '_plans' not in G.__dict__
        assert type(G) is type(F) and G.dim == 1 and G.abs and torch.equal(G.win, F.win) and torch.equal(G.freqs, F.freqs)
    P = ops.FFTPlan(1000, torch.float64, 'cuda')
    P.__dict__['_tw'] = {False: torch.zeros(3)}
    Q = pickle.loads(pickle.dumps(P))
    assert '_tw' not in Q.__dict__ and Q.radix == P.radix and Q.N == 1000 and Q.dtype == torch.float64
    assert list(Q._radix_c) == P.radix


def test_radix_lists():
    from bayeslim_amd import ops
    for N in range(1, ops.FFT_MAX_N + 1):
        r = ops.fft_radices(N)
        assert int(np.prod(r, dtype=np.int64)) == N, N
        assert len(r) <= 12 and all(p >= 2 for p in r)
        # radix 4 first while two factors of 2 are left, then at most one 2, then odd primes ascending
        n4 = len([p for p in r if p == 4])
        assert r[:n4] == [4] * n4 and r.count(2) <= 1 and (2 not in r or r[n4] == 2)
        rest = r[n4 + r.count(2):]
        assert rest == sorted(rest) and all(p % 2 == 1 and fc.sopfr(p) == p for p in rest), (N, r)
        v2 = (N & -N).bit_length() - 1
        assert n4 == v2 // 2 and r.count(2) == v2 % 2
    assert ops.fft_radices(1) == [] and ops.fft_radices(256) == [4] * 4 and ops.fft_radices(130) == [2, 5, 13]
    assert ops.fft_radices(4093) == [4093] and ops.fft_radices(1000) == [4, 2, 5, 5, 5]
    with pytest.raises(ValueError):
        ops.fft_radices(0)
    with pytest.raises(ValueError):
        ops.FFTPlan(4097, torch.float32, 'cuda')
    with pytest.raises(TypeError):
        ops.FFTPlan(8, torch.float16, 'cuda')


@pytest.mark.parametrize('N', [1, 2, 37, 256, 1000, 4093, 4096])
def test_twiddle_table(N):
    from bayeslim_amd import ops
    j = np.arange(N)
    for inverse, sign in ((False, -1.0), (True, 1.0)):
        t = ops.fft_twiddles(N, inverse)
        assert t.dtype == np.complex128 and t.shape == (N,)
        assert np.abs(t - np.exp(sign * 2j * np.pi * j / N)).max() <= 2e-16
        assert np.abs(np.abs(t) - 1).max() <= 3e-16 and t[0] == 1
    assert np.array_equal(ops.fft_twiddles(N, True), ops.fft_twiddles(N, False).conj())


def test_epilogue_names_and_scale():
    from bayeslim_amd import ops
    m = ops.fft_epilogue_mask
    assert [m('none'), m('abs'), m('peaknorm'), m('square'), m('peak')] == [0, 1, 2, 4, 8]
    assert m('abs+peaknorm+square') == 7 and m('square+abs') == 5 and m('abs+peak') == 9
    with pytest.raises(ValueError):
        m('log')
    assert ops.fft_scale(16, False, None) == 1.0 and ops.fft_scale(16, True, None) == 1 / 16
    assert ops.fft_scale(16, False, 'forward') == 1 / 16 and ops.fft_scale(16, True, 'forward') == 1.0
    assert ops.fft_scale(16, True, 'ortho') == 0.25 and ops.fft_scale(16, False, 'backward') == 1.0
    with pytest.raises(ValueError):
        ops.fft_scale(16, False, 'unitary')


def test_entry_point_rejects_bad_arguments_without_launching():
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)      # non-null dummy; never dereferenced on a rejected call
    r44 = (ctypes.c_int * 2)(4, 4)
    r35 = (ctypes.c_int * 2)(3, 5)

    def call(dtype=0, x=one, tw=one, win=None, wst=0, radix=r44, nr=2, N=16, nlines=3, inv=0, si=0, so=0, scale=1.0, epi=0, y=one):
        return lib.rime_fft_apply(dtype, x, tw, win, wst, radix, nr, N, nlines, inv, si, so, scale, epi, 0.0, 1.0, y, None)

    assert call(nlines=0) == 0                                  # valid, no line: nothing to do, no launch
    assert call(N=0, nr=0) == -1 and call(N=-4) == -1           # N < 1
    assert call(N=4097, radix=(ctypes.c_int * 1)(4097), nr=1) == -1
    assert call(N=8192, radix=(ctypes.c_int * 2)(2, 4096), nr=2) == -1
    assert call(dtype=2) == -1 and call(dtype=-1) == -1         # unknown dtype
    assert call(epi=16) == -1 and call(epi=-1) == -1            # unknown epilogue
    assert call(x=None) == -1 and call(y=None) == -1 and call(tw=None) == -1        # null data pointers
    assert call(radix=r35) == -1                                # product 15, N 16
    assert call(radix=r44, nr=1) == -1                          # product 4
    assert call(radix=(ctypes.c_int * 2)(16, 1), nr=2) == -1    # a radix below 2
    assert call(radix=None, nr=2) == -1 and call(nr=-1) == -1 and call(nr=13) == -1
    assert call(N=1, nr=0, nlines=0) == 0 and call(N=1, nr=0, si=1) == -1
    assert call(si=16) == -1 and call(so=-1) == -1              # shifts outside [0, N)
    assert call(nlines=-1) == -1 and call(inv=2) == -1 and call(wst=3) == -1


def test_fft_apply_refuses_cpu_tensors():
    from bayeslim_amd import ops
    plan = ops.FFTPlan(8, torch.float32, 'cuda')
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ops.fft_apply(torch.zeros(2, 8, dtype=torch.complex64), plan)


def test_fft_kernels_use_no_scratch():
    """the gfx950 assembly of THIS build of csrc/fft.hip: two kernels (f32, f64), no private segment"""
    _, kernels, sizes = kernel_asm.read('fft')
    assert len(kernels) == 2 and all('fft_kernel' in k for k in kernels), kernels
    assert len(sizes) == 2 and max(sizes) == 0, sizes


@pytest.mark.parametrize('N', [n for n in fc.SIZES if n > 1])
def test_reference_float32_transform_meets_the_bound(N):
    """the bound of fft_common is one the reference's own transform (torch.fft on CPU complex64) meets, on noise plus a
    strong tone, with a window, in both directions"""
    rng = np.random.default_rng(N)
    x = fc.tone_input(rng, (3, N), amp=8.0, cdtype=torch.complex64)
    w = fc.window_vec(rng, N).to(torch.float32)
    for ifft, norm in ((False, None), (True, None), (False, 'ortho')):
        y32 = torch.fft.ifft(x * w, norm=norm) if ifft else torch.fft.fft(x * w, norm=norm)
        y64 = fc.oracle_linear(x, ifft=ifft, win=w, norm=norm)
        B = fc.bound(x, N, torch.float32, ifft=ifft, win=w, norm=norm)
        ratio = float(((y32.to(torch.complex128) - y64).abs() / B).max())
        print('N %d ifft %d norm %s: reference f32 error / bound = %.3f' % (N, ifft, norm, ratio))
        assert ratio <= 1.0, (N, ifft, norm, ratio)


def test_average_data_against_the_reference():
    from bayeslim_amd import dataset
    g = fc.golden()
    d, idx = g['avg_x'], g['avg_index']
    a, sw, ac = dataset.average_data(d, 1, idx, 3)
    assert ac is None and float((a - g['avg0_data']).abs().max()) < 1e-14 and torch.allclose(sw.double(), g['avg0_wgts'].double())
    a, sw, ac = dataset.average_data(d, -2, idx, 3, wgts=g['avg_w'], cov=g['avg_cov'])
    for mine, key in ((a, 'avg1_data'), (sw, 'avg1_wgts'), (ac, 'avg1_cov')):
        assert mine.shape == g[key].shape and float((mine - g[key]).abs().max()) < 1e-14, key
    a, sw, _ = dataset.average_data(d, 1, idx, 3, wgts=g['avg2_w'])
    assert float((a - g['avg2_data']).abs().max()) < 1e-14 and float((sw - g['avg2_wgts']).abs().max()) < 1e-14
    a, sw, ac = dataset.average_data(d, -2, idx, 3, wgts=g['avg_w'], cov=g['avg_cov'], truncate=True)
    for mine, key in ((a, 'avg3_data'), (sw, 'avg3_wgts'), (ac, 'avg3_cov')):
        assert mine.shape == g[key].shape and float((mine - g[key]).abs().max()) < 1e-14, key


def test_bl_average_against_the_reference(f64):
    g = fc.golden()
    vd = fc.hex7_visdata(g)
    d0 = vd.data.clone()
    av = vd.bl_average()
    assert av is not vd and torch.equal(vd.data, d0) and vd.Nbls == 21
    assert np.array_equal(np.asarray(av.bls), g['blavg_bls'].numpy())
    assert av.data.shape == g['blavg_data'].shape and float((av.data - g['blavg_data']).abs().max()) < 1e-14
    assert av.flags is None and av.icov is None and av.Nbls == 9
    reds = [[], [], []]
    for i, a, b in g['blavg_reds'].tolist():
        reds[i].append((a, b))
    vd = fc.hex7_visdata(g, flags=True, icov=True)
    av = vd.bl_average(reds=reds)
    assert np.array_equal(np.asarray(av.bls), g['blavg2_bls'].numpy())
    assert float((av.data - g['blavg2_data']).abs().max()) < 1e-14
    assert torch.equal(av.flags, g['blavg2_flags'])
    assert float((av.icov / g['blavg2_icov'] - 1).abs().max()) < 1e-13
    out = vd.bl_average(reds=reds, inplace=True)
    assert out is vd and vd.Nbls == 3
