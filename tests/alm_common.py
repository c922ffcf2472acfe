"""
Reference, error bound and case table of the alm2pix tests (csrc/alm.hip); shared by tests/test_alm_host.py (CPU),
tests/test_alm_gpu.py and tests/alm_switch_child.py.

THE REFERENCE restates the two formula lines at the top of alm.hip on the real K axis of the kernels,

    fwd : out[r, j]  = sum_c ( are[r,c] Yre[c,j] - aim[r,c] Yim[c,j] )          K = 2 Ncoeff, k = (c, re | im)
    bwd : galm[r, c] = sum_j gout[r, j] * conj(Ylm[c, j])                        K = Npix, one real sum per component

as plain numpy matrix products: in float64 for the float32 paths, in numpy's extended precision (longdouble, 2^-64 on x86)
for the float64 path, whose own unit roundoff a float64 reference would share.  The inputs are rounded to the working
precision BEFORE the reference sees them.  Next to every result stands S = sum_k |a_k| |Y_k|, the scale of its bound.

THE BOUND is elementwise, per path, with u = 2^-53 (float64) or 2^-24 (float32).

  float64 VALU, exact-f32 matrix cores:     (K + c) u S
      K products, each rounded at most once (none where the kernel fuses multiply and add), summed in SOME order -- lanes,
      waves, pixel splits and the reduce kernel only choose the order -- so every term passes through at most K - 1
      additions; c = C_RED = 4 stands for the second-order terms and the zero partials of empty splits.

  f16 split (register-staged, LDS-DMA ring, packed):
      3 * 2^-20 S  +  2^-24 ( sum_k |a_k| / y_scale  +  sum_k |Y_k| / s_r )  +  (K + c) u32 S
      Both operands are scaled by powers of two (exact): A = a s_r with the row scale s_r of split_rows_kernel /
      row_scale_alm_kernel (max |A| in [2^12, 2^13), exponent clamped to +-100; row_scale() below restates it), B = Y y_scale.
      split2h cuts x into hi = rtz_f16(x) and lo = rtz_f16(x - hi).  An f16 significand has 11 bits, so |x - hi| < 2^-10 |x|,
      the remainder is exact in float32, and |x - hi - lo| < 2^-10 |x - hi| < 2^-20 |x| while lo is a normal f16; below the
      normal range the f16 grid has the spacing 2^-24, which is then the error: eps(x) <= max(2^-20 |x|, 2^-24).
      Truncation never grows a magnitude, |hi + lo| <= |x| and |lo| <= 2^-10 |x|.  The matrix cores form
      Ah Bh + Ah Bl + Al Bh (ALM_MFMA triples), that is A B - Al Bl - eps(A) B - (Ah + Al) eps(B):
          |Al Bl|               <= 2^-20 |A| |B|                       the dropped product
          |eps(A) B|            <= 2^-20 |A| |B| + 2^-24 |B|
          |(Ah + Al) eps(B)|    <= 2^-20 |A| |B| + 2^-24 |A|
      Summed over k and divided by s_r y_scale (the kernels multiply by inv_scale[row] / y_scale, exact) this is the first
      two terms.  The f16 x f16 products are exact in float32 (22 bits); the accumulation in float32 is counted as one
      rounding per contracted index, (K + c) u32 S, the figure the exact-f32 path has too.  That is an assumption about
      the matrix core: the three instructions of a 16-index step may round 16 times between them (four-term sums rounded
      once each would make 12); a core that rounded after every single product would need 3 K.
      Float32 paths add K * 2^-126 for operands, products and results in the subnormal range of float32, which the
      matrix cores may flush.

The accumulation term alone reaches 2^-11 S at K = 2^13.  The largest relative size a lo image can have is 2^-10, so from
K of about 2^14 on a lost lo image is INSIDE the bound whatever the data: tests/test_alm_host.py shows for every case and
direction below that K that losing either lo image, a row scale wrong by a factor of two and a dropped K tail all leave
the bound, and that the numpy emulation of the split itself stays inside its first two terms.

THE DATA (draw): row r of alm / gout has the amplitude 2^e_r, e_r spread evenly over -80 .. 80 (one row: 2^0); row R // 2
is all zero; the LAST row has one nonzero entry, in its last k (the imaginary part of the last coefficient / the last
pixel), of value XS = 1 + 2^-10 - 2^-23, whose lo image is as large as a lo image gets (0.9985 * 2^-10 of it).  Ylm entries are
normal draws times 2^(-30 v), v uniform in [0, 1], and Ylm[last coefficient, last pixel] = XS (1 + i) / 4, so that the one
product of the last row carries a large lo image on either side.
"""
import functools
import zlib

import numpy as np

U = {'f64': 2.0 ** -53, 'f32': 2.0 ** -24}
CDT = {'f64': np.complex128, 'f32': np.complex64}
RDT = {'f64': np.float64, 'f32': np.float32}
C_RED = 4
TINY32 = 2.0 ** -126
XS = 1.0 + 2.0 ** -10 - 2.0 ** -23

# kernel families as rime_alm2pix_plan reports them (include/rime_hip.h)
F64_VALU, F32_MFMA, F16_REG, F16_DMA, PACKED4, PACKED8 = range(6)
FAMILY = ['f64 VALU', 'exact-f32 MFMA', 'f16-split register-staged', 'f16-split LDS-DMA ring', 'packed 4-wave', 'packed 8-wave']

# mode -> (precision, y_scale > 0, packed): how tests/test_alm_gpu.py runs every case
MODES = {'f64': ('f64', False, False), 'exact': ('f32', False, False), 'split': ('f32', True, False), 'packed': ('f32', True, True)}

# ------------------------------------------------------------------------------------------------ the case table
# (R, Ncoeff, Npix, the branch the case is there for)
CASES = [
    (1, 1, 1, 'MT 1, one row; every extent a tail: one K step, one pixel, one coefficient'),
    (32, 5, 2, 'MT 1 full row tile; two pixels: the ring kernels with a single chunk'),
    (33, 33, 31, 'MT 2 lower edge; 32-coefficient chunk + 1; odd pixels below one tile'),
    (64, 127, 33, 'MT 2 full; 128-coefficient block - 1; 32-pixel tile + 1, odd'),
    (65, 128, 127, 'MT 4 lower edge; exactly one 128-coefficient block; odd pixels below 128'),
    (128, 129, 129, 'MT 4 full; 128-coefficient block + 1: two coefficient tiles; 128-pixel block + 1'),
    (129, 257, 1110, 'two row tiles, the second with ONE row; 256-coefficient block + 1; even pixels: ring kernels'),
    (200, 257, 1111, 'two row tiles, ragged second; odd pixels: register-staged backward'),
    (200, 5, 1110, 'two row tiles at a short coefficient axis (forward K = 10 < one K step)'),
    (1, 257, 1111, 'one row against the long axes'),
    (33, 129, 1110, 'MT 2 ring kernel over two coefficient tiles'),
    (64, 33, 2, 'MT 2 with two pixels'),
    (129, 1, 31, 'two row tiles, one coefficient'),
    (65, 127, 1, 'MT 4, one pixel: backward K = 1'),
    (32, 128, 129, 'MT 1 at the 128 edges'),
    (128, 5, 33, 'MT 4 full at short axes'),
]
# long-row split of the row operand (R * L >= 2^20 and Rpad % 64 == 0), and the same R just below the threshold
LONG_CASES = [
    (65, 9, 16134, 'backward long rows, L % 4 = 2: misaligned rows, padding rows r >= R, granule tail; even: ring kernel'),
    (65, 9, 16133, 'backward long rows, odd pixels: register-staged kernel'),
    (65, 9, 16130, 'just below the backward threshold, even'),
    (65, 9, 16131, 'just below the backward threshold, odd'),
    (33, 15889, 130, 'forward long rows (L = 2 Ncoeff = 31778, L % 4 = 2, 31 padding rows)'),
    (33, 15886, 130, 'just below the forward threshold'),
]
# forced split counts: RIME_ALM_BWD_SPLITS = 1, 2, 3 (pixel chunks dealt cyclically), RIME_ALM_FWD_SPLITS = 1, 2, 3
FORCED_BWD = [(33, 129, 1650), (33, 129, 1651), (129, 129, 1650), (129, 129, 1651)]
FORCED_FWD = [(65, 100, 129)]
FORCED_S = (1, 2, 3)
# the switches read once per process (tests/alm_switch_child.py)
SWITCH_CASES = [(65, 129, 1110), (65, 129, 1111), (129, 129, 1110), (129, 129, 1111)]


def case_id(c):
    return '%dx%dx%d' % tuple(c[:3])


# ------------------------------------------------------------------------------------------------ the small formulas
def mt(R):
    return 4 if R > 64 else (2 if R > 32 else 1)


def rpad(R):
    m = mt(R) * 32
    return (R + m - 1) // m * m


def long_rows(R, L):
    return rpad(R) % 64 == 0 and R * L >= 1 << 20


def ksteps(K):
    return (K + 15) // 16


def deal(nchunk, S):
    """chunks split s runs when chunks are dealt cyclically: s, s + S, ..."""
    return [(nchunk - s + S - 1) // S if s < nchunk else 0 for s in range(S)]


def bwd_chunks(Npix, wide):
    """ring chunks of the backward: 2 K steps (4-wave kernels, K steps padded to a whole chunk), 1 K step (8-wave)"""
    n = ksteps(Npix)
    return n if wide else (n + 1) // 2


def bwd_max_splits(Npix):
    return max(1, ksteps(Npix) // 32)


def fwd_packed_chunks(Ncoeff):
    """chunks of 4 K steps of the packed forward (K steps padded to a whole chunk)"""
    return (ksteps(2 * Ncoeff) + 3) // 4


def fwd_packed_deal(Ncoeff, S):
    n = fwd_packed_chunks(Ncoeff)
    per = (n + S - 1) // S
    return [max(0, min(n, (s + 1) * per) - s * per) for s in range(S)]


def exact_bwd_splits(R, Ncoeff, Npix):
    blocks = ((Ncoeff + 15) // 16) * (rpad(R) // (mt(R) * 32))
    S = (2048 + blocks * mt(R) - 1) // (blocks * mt(R))
    return max(1, min(S, max(1, Npix // 1024)))


def row_scale(X):
    """the power of two of split_rows_kernel / row_scale_alm_kernel per row of X (float32 [R, L]), in float32 as there"""
    m = np.abs(X.astype(np.float32)).max(axis=1)
    with np.errstate(divide='ignore', over='ignore'):
        e = np.floor(np.log2(np.float32(8192.0) / m, dtype=np.float32))
    e = np.clip(e, -100.0, 100.0)
    return np.where(m > 0, np.exp2(e.astype(np.float64)), 1.0)


def y_scale(Y):
    """ops._ylm_scale: the power of two bringing max |Ylm| to [2^10, 2^11)"""
    amax = float(np.abs(Y).max())
    return float(2.0 ** np.floor(np.log2(2048.0 / amax))) if amax > 0 and np.isfinite(amax) else 1.0


# ------------------------------------------------------------------------------------------------ data
def draw(R, Ncoeff, Npix, prec, seed=0):
    """alm [R, Ncoeff] complex, Ylm [Ncoeff, Npix] complex, gout [R, Npix] real, rounded to the working precision"""
    rng = np.random.default_rng(zlib.crc32(b'alm %d %d %d %d' % (R, Ncoeff, Npix, seed)))
    amp = np.exp2(np.round(np.linspace(-80, 80, R))) if R > 1 else np.ones(1)
    alm = (rng.normal(size=(R, Ncoeff)) + 1j * rng.normal(size=(R, Ncoeff))) * amp[:, None]
    gout = rng.normal(size=(R, Npix)) * amp[:, None]
    Y = (rng.normal(size=(Ncoeff, Npix)) + 1j * rng.normal(size=(Ncoeff, Npix))) * np.exp2(-30 * rng.uniform(size=(Ncoeff, Npix)))
    Y[-1, -1] = XS * (1 + 1j) / 4
    if R >= 3:
        alm[R // 2] = 0
        gout[R // 2] = 0
        alm[-1] = 0
        alm[-1, -1] = 1j * XS
        gout[-1] = 0
        gout[-1, -1] = XS
    return alm.astype(CDT[prec]), Y.astype(CDT[prec]), gout.astype(RDT[prec])


# ------------------------------------------------------------------------------------------------ reference
def real_operands(alm, Y, wide):
    """the real GEMM operands: A [R, 2 Ncoeff] with the imaginary parts negated, Yk [2 Ncoeff, Npix], k = (c, re | im)"""
    R, Nc = alm.shape
    A = np.stack([alm.real, -alm.imag], axis=-1).reshape(R, 2 * Nc).astype(wide)
    Yk = np.stack([Y.real, Y.imag], axis=1).reshape(2 * Nc, Y.shape[1]).astype(wide)
    return A, Yk


def forward(alm, Y, prec):
    """out [R, Npix], S, and the two 1-norms of the floor terms (sum_k |a_k| per row, sum_k |Y_k| per column)"""
    wide = np.longdouble if prec == 'f64' else np.float64
    A, Yk = real_operands(alm, Y, np.float64)
    S = np.abs(A) @ np.abs(Yk)                         # (the scale of the bound needs no more than float64)
    return A.astype(wide) @ Yk.astype(wide), S, np.abs(A).sum(1), np.abs(Yk).sum(0)


def backward(gout, Y, prec):
    """galm [R, Ncoeff] complex (a pair of real sums), S per component (complex container), and the 1-norms"""
    wide = np.longdouble if prec == 'f64' else np.float64
    g = gout.astype(np.float64)
    Yre, Yim = Y.real.astype(np.float64), Y.imag.astype(np.float64)
    re, im = g.astype(wide) @ Yre.T.astype(wide), -(g.astype(wide) @ Yim.T.astype(wide))
    S = np.abs(g) @ np.abs(Yre).T + 1j * (np.abs(g) @ np.abs(Yim).T)
    ysum = np.abs(Yre).sum(1) + 1j * np.abs(Yim).sum(1)
    return (re, im), S, np.abs(g).sum(1), ysum


@functools.lru_cache(maxsize=None)
def case_data(R, Ncoeff, Npix, prec):
    """inputs and both references of one case, computed once and shared (read only)"""
    alm, Y, gout = draw(R, Ncoeff, Npix, prec)
    for x in (alm, Y, gout):
        x.setflags(write=False)
    return dict(alm=alm, Y=Y, gout=gout, fwd=forward(alm, Y, prec), bwd=backward(gout, Y, prec),
                ys=y_scale(Y) if prec == 'f32' else 0.0,
                srow_fwd=row_scale(np.stack([alm.real, alm.imag], -1).reshape(R, -1)) if prec == 'f32' else None,
                srow_bwd=row_scale(gout) if prec == 'f32' else None)


# ------------------------------------------------------------------------------------------------ bound
def bound_accum(S, K, prec):
    b = (K + C_RED) * U[prec] * S
    return b + K * TINY32 if prec == 'f32' else b


def bound_split(S, asum, ysum, srow, ys):
    """the split part of the f16 bound: 3 * 2^-20 S + 2^-24 (sum |a| / y_scale + sum |Y| / s_r); S [R, N], asum [R], ysum [N]"""
    return 3 * 2.0 ** -20 * S + 2.0 ** -24 * (asum[:, None] / ys + ysum[None, :] / srow[:, None])


def bound(S, K, prec, split=None):
    """split: None (float64 VALU, exact f32) or (asum, ysum, srow, ys) for the f16-split families"""
    b = bound_accum(S, K, prec)
    return b if split is None else b + bound_split(S, *split)


def check(got, ref, bnd, what):
    """worst error / bound of one real array, printed; every element finite and inside the bound"""
    got = np.asarray(got)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), what + ': non-finite output'
    err = np.abs(got.astype(ref.dtype) - ref).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err > 0, err / bnd, 0.0)
    worst = float(ratio.max())
    print('%s: worst error / bound %.3f' % (what, worst))
    assert worst <= 1.0, '%s: worst error / bound %.3f at %s' % (what, worst, np.unravel_index(ratio.argmax(), ratio.shape))
    return worst


def check_forward(out, d, K, prec, split, what):
    ref, S, asum, ysum = d['fwd']
    sp = (asum, ysum, d['srow_fwd'], d['ys']) if split else None
    return check(out, ref, bound(S, K, prec, sp), what + ' forward')


def check_backward(galm, d, K, prec, split, what):
    (re, im), S, gsum, ysum = d['bwd']
    w = []
    for name, got, ref, s, ys1 in (('re', galm.real, re, S.real, ysum.real), ('im', galm.imag, im, S.imag, ysum.imag)):
        sp = (gsum, ys1, d['srow_bwd'], d['ys']) if split else None
        w.append(check(got, ref, bound(s, K, prec, sp), '%s adjoint (%s)' % (what, name)))
    return max(w)


# ------------------------------------------------------------------------------------------------ emulation of the split
def split_f16(x):
    """split2h on float64 copies of float32 values: hi = x cut to an 11-bit significand on the f16 grid (normal down to 2^-14,
    spacing 2^-24 below), toward zero; lo = the same cut of x - hi"""
    def rtz(v):
        _, e = np.frexp(v)
        qe = np.maximum(e - 11, -24)
        return np.ldexp(np.trunc(np.ldexp(v, -qe)), qe)
    hi = rtz(x)
    return hi, rtz(x - hi)


def emulate(A, B, srow, ys, lose=None):
    """(hi hi + hi lo + lo hi) / (s_r y_scale) in float64 for A [R, K], B [K, N]; `lose`: 'a_lo', 'b_lo' (a lost lo image),
    'scale' (the row scale applied to the result a factor of two off), 'tail' (the last K index dropped)"""
    A, B = A.astype(np.float64), B.astype(np.float64)
    assert np.abs(A * srow[:, None]).max(initial=0) < 2.0 ** 13 and np.abs(B * ys).max(initial=0) < 2.0 ** 11
    ah, al = split_f16(A * srow[:, None])
    bh, bl = split_f16(B * ys)
    if lose == 'a_lo':
        al = al * 0
    if lose == 'b_lo':
        bl = bl * 0
    if lose == 'tail':
        ah, al, bh, bl = ah[:, :-1], al[:, :-1], bh[:-1], bl[:-1]
    acc = ah @ bh + ah @ bl + al @ bh
    return acc / (srow[:, None] * (2.0 if lose == 'scale' else 1.0)) / ys
