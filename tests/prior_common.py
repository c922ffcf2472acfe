"""
What the tests of the log-prior kernel (csrc/prior.hip) share: a float64 oracle written from the laws, the case tables and
the floating-point error bound.  No GPU is needed to import this.

Laws, per element x (m mean, s scale, l / u bounds, c coefficient; an absent bound drops its term):
    laplace        t = -|r| / s, r = x - m; side 'upper': r < 0 -> 0, 'lower': r > 0 -> 0      d = -sign(r) / s, 0 at r == 0
    taper_sigmoid  t = logsig(z1) + logsig(z2), z1 = c (x - l), z2 = -c (x - u)                 d = c sig(-z1) - c sig(-z2)
    taper_tanh     t = log tanh z1 + log tanh z2 (NaN for z < 0)                                d = 2c / sinh 2 z1 - 2c / sinh 2 z2
value = sum t, gradient element = d.

The bound.  The inputs of a case are exactly representable in the working type T (they are drawn in float32), so an error of
a term comes from roundings in T (unit eps_T = 2^-23 or 2^-52; one rounding is eps_T / 2 relative) and from the device's
exp / expm1 / log / log1p, and is a multiple K of eps_T times |t| + |z t'(z)|: the second part is what a relative error of z,
formed with two roundings, does to the term.  Counting the operations of prior.hip (U_f: error of device function f in ulp):
  sigmoid value   e = exp(-|z|), L = log1p(e), t = min(z, 0) - L, and e / (1 + e) <= L <= |t|:
                  (U_exp + U_log1p + 1/2) |t| + 1 |z t'|, and 1/2 |t| for the sum of the two terms
  sigmoid deriv.  c (e or 1) / (1 + e): (2 U_exp + 3/2) |d_j| + 1 |z d_j'|, 1/2 for the sum of the two, 1/2 for g d
  tanh value      q = exp(-2z), em = -expm1(-2z), p = 1 + q;  z < 0.55: log(em / p), |z t'| = 2z / sinh 2z >= 0.82, so the
                  relative error U_expm1 + U_exp / 2 + 1 of em / p is at most that over 0.82 times |z t'|, and U_log |t|;
                  z >= 0.55: a = -2q / p (1.5 U_exp + 1), w = 1 + a in [1/2, 1] so that w - 1 is exact, log(w) a / (w - 1)
                  (log1p(a) / a changes by at most 0.45 eps over the rounding of w): (U_log + 1.5 U_exp + 2.5) |t|
  tanh deriv.     2c 2q / (em p): (1.5 U_exp + U_expm1 + 2) |d_j| + 1 |z d_j'|, + 1/2 + 1/2 as above
  laplace         one rounding each for x - m and the division: 1 |t|; the derivative 1/2 |d| + 1/2 for g d
Underflow: an exp below the smallest normal number of T (TINY) may come out as 0, an absolute error of at most TINY in e or
q, which moves a term by at most 2 TINY and its derivative by at most 4 c TINY; 4 TINY and 4 c TINY per term are added.
The summed value adds the double accumulation, N eps_64 sum |t|, and the rounding of the sum to T, eps_T / 2 |sum t|.  The
oracle itself works in float64 with numpy's functions: its own error has the same form with eps_64, and is added.

No figure for the error of the device functions is documented on the build machine (the ROCm installation carries no
accuracy table of the HIP math library), so each U below is twice the largest error of a one-off comparison on an MI355X
against long double over the arguments the kernel passes (2^21 arguments each, half of them spaced logarithmically):
                 measured, ulp      float    double
    exp on [-87, 0] / [-708, 0]     0.97     0.86        (float: prior.hip's own exp, not expf -- see there)
    expm1 on [-40, 0]               0.85     1.13
    log on (0, 1]                   2.14     1.68
    log1p on [0, 1]                 1.06     1.95
"""
import numpy as np
import torch

EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
TINY = {torch.float32: 2.0 ** -126, torch.float64: 2.0 ** -1022}
# twice the measured errors of the device functions, in ulp (the table above)
ULP = {torch.float32: dict(exp=2 * 0.97, expm1=2 * 0.85, log=2 * 2.14, log1p=2 * 1.06),
       torch.float64: dict(exp=2 * 0.86, expm1=2 * 1.13, log=2 * 1.68, log1p=2 * 1.95)}

KINDS = ('laplace', 'taper_sigmoid', 'taper_tanh')
SIDES = ('both', 'upper', 'lower')
SIZES = (1, 3, 63, 64, 65, 255, 257, 4097)
BOUNDS = ('both', 'lower', 'upper')
ALPHAS = (1.0, 1e4)
LO, HI = -1.5, 2.5                     # the bounds of the taper cases: HI - LO = 4, so that alpha / (HI - LO) is exact


def _f32(a):
    """float64 array of values that float32 holds exactly"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _tail(shape, mode):
    """shape of an operand: () for 'scalar', x's for 'full', the trailing axes of x whose product is `mode` for an int"""
    if mode in ('scalar', 'full'):
        return () if mode == 'scalar' else tuple(shape)
    k, tail = 1, ()
    while k < mode:
        tail = (shape[len(shape) - len(tail) - 1],) + tail
        k *= tail[0]
    assert k == mode, (shape, mode)
    return tail


def laplace_case(N, seed=0, shape=None, mode='scalar'):
    """x, mean, scale for N elements (or `shape`); mode 'scalar', 'full' or an int: operands over that many trailing
    elements; every eighth residual is exactly 0"""
    rng = np.random.default_rng(1000 + seed)
    shape = (N,) if shape is None else shape
    N = int(np.prod(shape))
    tail = _tail(shape, mode)
    m = _f32(rng.normal(size=tail))
    s = _f32(rng.uniform(0.5, 2.0, size=tail))
    x = _f32(rng.normal(size=shape) * 2)
    x = np.where(np.arange(N).reshape(shape) % 8 == 0, np.broadcast_to(m, shape), x)
    return x, m, s


def taper_case(N, kind, bounds='both', alpha=1.0, seed=0, shape=None, mode='scalar'):
    """x, lower, upper, coeff; x strictly inside the bounds for 'taper_tanh', reaching beyond them for 'taper_sigmoid'"""
    rng = np.random.default_rng(2000 + seed)
    shape = (N,) if shape is None else shape
    tail = _tail(shape, mode)
    jitter = _f32(rng.integers(-2, 3, size=tail) / 4.0)              # operands that differ along the period, exact in float32
    lo, hi = LO + jitter, HI + jitter
    c = _f32(np.full(tail, alpha / (HI - LO)))
    span = (0.001, 0.999) if kind == 'taper_tanh' else (-0.25, 1.25)
    # half of the elements sit in the taper whatever alpha is: at 10^-0.3 ... 10^-5 of the range from one of the bounds
    near, sel = 10.0 ** -rng.uniform(0.3, 5.0, size=shape), rng.integers(0, 4, size=shape)
    f = np.where(sel == 0, near, np.where(sel == 1, 1 - near, rng.uniform(*span, size=shape)))
    x = _f32(lo + (hi - lo) * f)
    if kind == 'taper_tanh':                                           # the rounding to float32 must not leave the bounds
        x = np.clip(x, _f32(lo + 2.0 ** -16), _f32(hi - 2.0 ** -16))
    return x, (lo if bounds in ('both', 'lower') else None), (hi if bounds in ('both', 'upper') else None), c


def _logsig(z):
    e = np.exp(-np.abs(z))
    t = np.minimum(z, 0) - np.log1p(e)
    t1 = np.where(z >= 0, e, 1.0) / (1 + e)                            # sig(-z) = t'(z)
    t2 = -e / (1 + e) ** 2                                             # t''(z)
    return t, t1, t2


def _logtanh(z):
    with np.errstate(all='ignore'):
        za = np.abs(z)
        q, em = np.exp(-2 * za), -np.expm1(-2 * za)
        p = 1 + q
        t = np.where(za < 0.55, np.log(em / p), np.log1p(-2 * q / p))
        t = np.where(z < 0, np.nan, t)
        t1 = np.sign(z) * 4 * q / (em * p)                             # 2 / sinh 2z
        t1 = np.where(z == 0, np.inf, t1)
        t2 = -8 * q * (1 + q * q) / (em * p) ** 2                      # -4 cosh 2z / sinh^2 2z
    return t, t1, t2


def oracle(kind, x, mean=None, scale=None, lower=None, upper=None, coeff=None, side='both'):
    """float64: dict of value (sum t), grad (d, x-shaped) and what the bound is made of, each x-shaped: abs_t = sum_j |t_j|,
    sens_t = sum_j |z_j t_j'|, abs_d = sum_j |d_j|, sens_d = sum_j |z_j d_j'|"""
    x = np.asarray(x, dtype=np.float64)
    if kind == 'laplace':
        r = x - mean
        if side == 'upper':
            r = np.where(r < 0, 0.0, r)
        elif side == 'lower':
            r = np.where(r > 0, 0.0, r)
        t = -np.abs(r) / scale + 0 * x
        d = -np.sign(r) / scale + 0 * x
        return dict(value=t.sum(), grad=d, abs_t=np.abs(t), sens_t=np.abs(t), abs_d=np.abs(d), sens_d=0 * x, under=0.0)
    f = _logsig if kind == 'taper_sigmoid' else _logtanh
    t = np.zeros_like(x)
    out = dict(grad=np.zeros_like(x), abs_t=np.zeros_like(x), sens_t=np.zeros_like(x), abs_d=np.zeros_like(x),
               sens_d=np.zeros_like(x))
    with np.errstate(all='ignore'):
        for bound, sign in ((lower, 1.0), (upper, -1.0)):
            if bound is None:
                continue
            z = sign * coeff * (x - bound)
            tj, t1, t2 = f(z)
            dj = sign * coeff * t1
            t = t + tj
            out['grad'] += dj
            out['abs_t'] += np.abs(tj)
            out['sens_t'] += np.abs(z * t1)
            out['abs_d'] += np.abs(dj)
            out['sens_d'] += np.abs(z * coeff * t2)
    out['value'] = t.sum()
    out['under'] = 4.0 * ((lower is not None) + (upper is not None)) * float(np.max(np.abs(coeff)))   # of TINY, per derivative
    return out


def constants(kind, dtype):
    """(K on |t|, K on |z t'|, K on |d_j|, K on |z d_j'|) of the docstring's count, in units of eps_T"""
    U = ULP[dtype]
    if kind == 'laplace':
        return 0.5, 0.5, 1.0, 0.0
    if kind == 'taper_sigmoid':
        return U['exp'] + U['log1p'] + 1.0, 1.0, 2 * U['exp'] + 2.5, 1.0
    return (max(U['log'], U['log'] + 1.5 * U['exp'] + 2.5) + 0.5, (U['expm1'] + U['exp'] / 2 + 1) / 0.82 + 1.0,
            1.5 * U['exp'] + U['expm1'] + 3.0, 1.0)


def bound(kind, dtype, orc, g=1.0):
    """(bound of |value - oracle value|, bound of |gradient - g oracle grad| per element) for a kernel working in `dtype`"""
    kt, kst, kd, ksd = constants(kind, dtype)
    eps, e64 = EPS[dtype], EPS[torch.float64]
    N = orc['grad'].size
    terms = 0 if kind == 'laplace' else 2
    bv = ((eps + e64) * (kt * orc['abs_t'].sum() + kst * orc['sens_t'].sum()) + N * e64 * orc['abs_t'].sum()
          + 0.5 * eps * abs(orc['value']) + 4 * terms * N * TINY[dtype])
    bg = abs(g) * ((eps + e64) * (kd * orc['abs_d'] + ksd * orc['sens_d']) + orc['under'] * TINY[dtype])
    return bv, bg


# ---- the recorded reference cases (tests/golden/prior.npz, written by tests/golden/make_golden_prior.py) --------------------
GOLDEN_N = 300


def golden_cases():
    """[(name, 'laplace' | 'taper', constructor keywords of the reference class, x)]: every side, one or both bounds, alpha
    1, 10 and 1e4, scalar and full operands; x inside the bounds, where the reference's log(sigmoid) and log(tanh) are finite"""
    cases = []
    for side in SIDES:
        for mode in ('scalar', 'full'):
            for density in (True, False):
                x, m, s = laplace_case(GOLDEN_N, seed=len(cases), mode=mode)
                cases.append(('laplace_%s_%s_%s' % (side, mode, 'density' if density else 'peak'), 'laplace',
                              dict(mean=m, scale=s, side=side, density=density), x))
    for kind in ('sigmoid', 'tanh'):
        for bounds in BOUNDS:
            for alpha in (1.0, 10.0, 1e4):
                for mode in ('scalar', 'full'):
                    x, lo, hi, _ = taper_case(GOLDEN_N, 'taper_tanh', bounds, alpha, seed=len(cases), mode=mode)
                    cases.append(('taper_%s_%s_a%g_%s' % (kind, bounds, alpha, mode), 'taper',
                                  dict(lower_bound=lo, upper_bound=hi, kind=kind, alpha=alpha), x))
    return cases
