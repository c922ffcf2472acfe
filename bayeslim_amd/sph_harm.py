"""
Spherical-harmonic forward model with the reference's API (sph_harm.py): `gen_lm` (:14-40),
`gen_sph2pix` for integer degree on the full sphere (:255-475), `AlmModel`
(:1244-1581) whose a_lm -> pixel product runs in the HIP kernel `rime_alm2pix_fwd/bwd`, and the
spherical Fourier-Bessel layer `gen_bessel2freq`, `sph_bessel_func`, `sph_bessel_kln` (:955-1241),
`SFBModel` and `sfb_binning` (:1851-2145) whose radial transform t_lmn -> a_lm(r) runs in the HIP
kernel `rime_sfb_fwd/bwd` (one launch for all degrees).

Out of scope (one-off host setup in the reference): cut-sky (cap / stripe)
non-integer-degree bases built from hypergeometric functions, HDF5 Ylm files; of the SFB layer
`SFBModel.least_squares` (needs the reference's linalg module) and boundary condition 3.  The comoving distance r of
every channel, an input of `SFBModel.setup_gln`, comes from `cosmology.Cosmology().f2r(freqs)`.
"""
import copy
import math

import numpy as np
import torch

from . import utils, ops
from .utils import _float, _cfloat, D2R


def gen_lm(lmax, real_field=True):
    """(2, Ncoeff) array of (l, m), m-major, m >= 0 for a real field (sph_harm.py:14-40)"""
    lm = [(l, m) for m in range(0 if real_field else -lmax, lmax + 1)
          for l in range(abs(m), lmax + 1)]
    return np.array(lm).T


def _norm_legendre(x, sth, lmax, mmax):
    """orthonormalised P~_lm(x) (incl. sqrt((2l+1)/4pi (l-m)!/(l+m)!) and the Condon-Shortley
    phase) for 0 <= m <= mmax, m <= l <= lmax, by upward recurrence in l; dict[(l, m)]"""
    out = {}
    pmm = np.full_like(x, math.sqrt(1.0 / (4 * math.pi)))
    for m in range(mmax + 1):
        if m > 0:
            pmm = -math.sqrt((2 * m + 1) / (2.0 * m)) * sth * pmm
        out[(m, m)] = pmm
        if m + 1 <= lmax:
            out[(m + 1, m)] = math.sqrt(2 * m + 3) * x * pmm
        for l in range(m + 2, lmax + 1):
            a = math.sqrt((4.0 * l * l - 1) / (l * l - m * m))
            b = math.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1) ** 2 - 1))
            out[(l, m)] = a * (x * out[(l - 1, m)] - b * out[(l - 2, m)])
    return out


def gen_sph2pix(theta, phi, l, m, separable=False, method='sphere', device=None, real=False,
                m_phasor=False, **kwargs):
    """
    Y_lm(theta, phi) matrix for integer l on the full sphere (theta colatitude [rad], phi
    [rad]).  Returns (Ylm, norm, alm_mult) like the reference (sph_harm.py:255-475):
    Ylm (Ncoeff, Npix) complex (or real part if real=True), or (Theta (Ncoeff, Ntheta),
    Phi (Ncoeff, Nphi)) if separable; alm_mult = 2 for m > 0 when negative m are truncated.
    """
    if method != 'sphere':
        raise NotImplementedError("only method='sphere' (integer degree) is built natively; "
                                  "cut-sky bases are out of scope")
    l = np.atleast_1d(np.asarray(l))
    m = np.atleast_1d(np.asarray(m))
    assert np.allclose(l, np.round(l)) and np.allclose(m, np.round(m)), 'integer l, m only'
    theta = np.atleast_1d(np.asarray(utils.tensor2numpy(theta), dtype=np.float64))
    phi = np.atleast_1d(np.asarray(utils.tensor2numpy(phi), dtype=np.float64))
    li, mi = l.astype(int), m.astype(int)
    N = _norm_legendre(np.cos(theta), np.sin(theta), int(li.max()), int(np.abs(mi).max()))
    H = np.empty((len(l), len(theta)))
    for k, (ll, mm) in enumerate(zip(li, mi)):
        h = N[(ll, abs(mm))]
        H[k] = h if mm >= 0 else (-1) ** abs(mm) * h      # Y_{l,-m} = (-1)^m conj(Y_lm)
    Phi = np.exp(1j * mi[:, None] * phi[None, :])
    if m_phasor:
        Phi = Phi * np.exp(1j * phi)[None, :]
    dtype = _float() if real else _cfloat()
    if separable:
        Y = (torch.as_tensor(H, dtype=dtype, device=device),
             torch.as_tensor(Phi.real if real else Phi, dtype=dtype, device=device))
    else:
        full = H * Phi
        Y = torch.as_tensor(full.real if real else full, dtype=dtype, device=device)
    norm = torch.ones(len(l))
    alm_mult = torch.ones(len(l), dtype=_float())
    if not np.any(mi < 0) and not real:
        alm_mult[mi > 0] *= 2
    if m_phasor and not real:
        alm_mult[mi == 0] *= 2
    return Y, norm, alm_mult


def inflate_Ylm(Ylm):
    """(Theta, Phi) -> full (Ncoeff, Ntheta*Nphi), theta-slow / phi-fast"""
    if isinstance(Ylm, (tuple, list)):
        T, P = Ylm
        return (T[:, :, None] * P[:, None, :]).reshape(T.shape[0], -1)
    return Ylm


class AlmModel:
    """
    f(theta, phi) = sum_lm a_lm Y_lm: params (..., Ncoeff) [complex, or (..., Ncoeff, 2) real
    view] -> map (..., Npix).  Ylm matrices are cached per angle set (sph_harm.py:1244-1581).
    """
    def __init__(self, l, m, default_kw=None, real_output=False, LM=None):
        self.l, self.m = l, m
        self.device = None
        self.default_kw = {} if default_kw is None else default_kw
        self.real_output = real_output
        self.LM = LM
        self.clear_Ylm_cache()
        self.clear_multigrid()

    def __call__(self, params, **kwargs):
        return self.forward_alm(params, **kwargs)

    def clear_Ylm_cache(self):
        self.Ylm_cache = {}

    def __getstate__(self):
        # pickle / deepcopy: the per-object conversion caches are keyed on id() of the ORIGINAL's Ylm tensors (and would carry
        # a second copy of each matrix along); the copy converts again on first use.  Ylm_cache itself travels, as in the
        # reference (sph_harm.py:1244-1581 keeps it on the object that io.write_pkl pickles)
        state = dict(self.__dict__)
        for k in ('_Ylm_pack_cache', '_Ylm_cast_cache', '_inflated'):
            state.pop(k, None)
        state['_inflated_key'] = None
        return state

    def clear_multigrid(self):
        self.multigrid = None
        self._multigrid_idx = None

    def set_multigrid(self, keys, idx=None):
        self.multigrid = list(keys)
        self._multigrid_idx = idx

    def forward_alm(self, params, Ylm=None, alm_mult=None, ignoreLM=False):
        """(params * alm_mult) @ Ylm [-> .real]  (sph_harm.py:1289-1372)"""
        if self.LM is not None and not ignoreLM:
            params = self.LM(params)
        if Ylm is None and self.multigrid is not None:
            outs = []
            for h in self.multigrid:
                c = self.Ylm_cache[h]
                outs.append(self.forward_alm(params, Ylm=c['Ylm'], alm_mult=c['alm_mult'], ignoreLM=True))
            out = torch.cat(outs, dim=-1)
            if self._multigrid_idx is not None:
                out = out.index_select(-1, self._multigrid_idx)
            return out
        if Ylm is None:
            Ylm, alm_mult = self.Ylm, self.alm_mult
        separable = isinstance(Ylm, (list, tuple))
        Yc = Ylm[1] if separable else Ylm
        if torch.is_complex(Yc) and not torch.is_complex(params):
            params = utils.viewcomp(params)
        if alm_mult is not None:
            params = params * alm_mult.to(params.device)
        if separable:
            # separable grids are small (Ntheta + Nphi columns): inflate once per Ylm object
            key = id(Ylm[0])
            if getattr(self, '_inflated_key', None) != key:
                self._inflated = inflate_Ylm(Ylm).contiguous()
                self._inflated_key = key
            Ylm = self._inflated
        if not params.is_cuda:
            raise RuntimeError('AlmModel.forward_alm needs GPU tensors (no CPU path)')
        if torch.is_complex(Ylm) and torch.is_complex(params):
            Yk = self._cast_Ylm(Ylm, params.dtype)
            if self.real_output:
                return ops.alm2pix(params, Yk)
            # complex output: Im(a Y) = Re((-i a) Y), so the rows [a ; -i a] go through the kernels in ONE
            # pass over Ylm (2 R rows) and the two halves are the real and imaginary parts
            both = ops.alm2pix(torch.stack([params, params * (-1j)]), Yk)
            return torch.complex(both[0], both[1])
        if not torch.is_complex(Ylm) and not torch.is_complex(params):
            # real Ylm (gen_sph2pix(real=True)): sum_c a_c Y_c = Re sum_k (a_2k - i a_2k+1)(Y_2k + i Y_2k+1) -- the
            # same kernels on a pair-packed copy of Ylm (built once per Ylm object, same bytes)
            Yp = self._packed_real_Ylm(Ylm, params.dtype)
            a = params
            if a.shape[-1] % 2:
                a = torch.cat([a, a.new_zeros(a.shape[:-1] + (1,))], dim=-1)
            a = a.reshape(a.shape[:-1] + (a.shape[-1] // 2, 2))
            return ops.alm2pix(torch.complex(a[..., 0], -a[..., 1]), Yp)
        # mixed real / complex operands (not produced by the reference's own constructors): plain GEMM
        out = torch.einsum('...i,ij->...j', params, Ylm.to(params.dtype))
        return out.real if (self.real_output and torch.is_complex(out)) else out

    def _packed_real_Ylm(self, Ylm, dtype):
        """real (Ncoeff, Npix) Ylm as complex (ceil(Ncoeff / 2), Npix): rows 2k + i rows 2k+1, cached per Ylm object"""
        cache = self.__dict__.setdefault('_Ylm_pack_cache', {})
        ent = cache.get(id(Ylm))
        if ent is None or ent[0] is not Ylm or ent[1] != Ylm._version or ent[2].real.dtype != dtype:
            if len(cache) > 8:
                cache.clear()
            Y = Ylm.to(dtype)
            if Y.shape[0] % 2:
                Y = torch.cat([Y, Y.new_zeros((1, Y.shape[1]))], dim=0)
            ent = (Ylm, Ylm._version, torch.complex(Y[0::2], Y[1::2]).contiguous())
            cache[id(Ylm)] = ent
        return ent[2]

    def _cast_Ylm(self, Ylm, dtype):
        """Ylm in the parameters' dtype, converted once per Ylm object (a complex128 matrix used with
        complex64 parameters would otherwise be re-cast -- 3.3 GB at C3 -- on every forward)"""
        if Ylm.dtype == dtype:
            return Ylm
        cache = self.__dict__.setdefault('_Ylm_cast_cache', {})
        ent = cache.get(id(Ylm))
        if ent is None or ent[0] is not Ylm or ent[1] != Ylm._version or ent[2].dtype != dtype:
            if len(cache) > 8:
                cache.clear()
            ent = (Ylm, Ylm._version, Ylm.to(dtype))
            cache[id(Ylm)] = ent
        return ent[2]

    @staticmethod
    def setup_angs(theta, phi, separable):
        if separable:
            ph, th = np.meshgrid(utils.tensor2numpy(phi), utils.tensor2numpy(theta), copy=False)
            return th.ravel(), ph.ravel()
        return theta, phi

    def setup_Ylm(self, theta, phi, Ylm=None, alm_mult=None, separable=False, generate=False,
                  cache=True, h=None, **kwargs):
        """attach (and optionally generate / cache) the transform for these angles [deg]
        (sph_harm.py:1408-1494)"""
        self.theta, self.phi = theta, phi
        if separable:
            self.theta_grid, self.phi_grid = theta, phi
            self.theta, self.phi = self.setup_angs(theta, phi, separable)
        if Ylm is None and generate:
            kw = dict(self.default_kw)
            kw.update(kwargs)
            th, ph = (self.theta_grid, self.phi_grid) if separable else (self.theta, self.phi)
            Ylm, _, alm_mult = gen_sph2pix(utils.tensor2numpy(th) * D2R, utils.tensor2numpy(ph) * D2R,
                                           self.l, self.m, separable=separable, device=self.device, **kw)
        self.Ylm, self.alm_mult, self.separable = Ylm, alm_mult, separable
        if cache:
            angs = (self.theta_grid, self.phi_grid) if separable else (theta, phi)
            self.set_Ylm(Ylm, angs, alm_mult=alm_mult, h=h)

    def get_Ylm(self, theta, phi, separable=False, h=None):
        h = h if h is not None else utils.arr_hash(theta)
        if h in self.Ylm_cache:
            c = self.Ylm_cache[h]
            self.Ylm, self.alm_mult = c['Ylm'], c['alm_mult']
            self.theta, self.phi = c['angs']
        else:
            self.setup_Ylm(theta, phi, cache=True, h=h, separable=separable, generate=True)
        self.separable = separable
        return self.Ylm, self.alm_mult

    def set_Ylm(self, Ylm, angs, alm_mult=None, h=None):
        h = h if h is not None else utils.arr_hash(angs[0])
        self.Ylm_cache[h] = dict(Ylm=Ylm, angs=angs, separable=isinstance(Ylm, (tuple, list)),
                                 alm_mult=alm_mult)
        return h

    def push(self, device):
        if not isinstance(device, torch.dtype):
            self.device = device
        mv = lambda y: tuple(utils.push(t, device) for t in y) if isinstance(y, (tuple, list)) \
            else utils.push(y, device)
        for c in self.Ylm_cache.values():
            c['Ylm'] = mv(c['Ylm']) if c['Ylm'] is not None else None
            if c['alm_mult'] is not None:
                c['alm_mult'] = utils.push(c['alm_mult'], device)
        if getattr(self, 'Ylm', None) is not None:
            self.Ylm = mv(self.Ylm)
        if getattr(self, 'alm_mult', None) is not None:
            self.alm_mult = utils.push(self.alm_mult, device)
        self._inflated_key = None
        self.__dict__.pop('_Ylm_cast_cache', None)
        if self.LM is not None:
            self.LM.push(device)


# ---------------------------------------------------------------------------------------
# spherical Fourier-Bessel radial basis (sph_harm.py:955-1241) -- host set-up, float64 numpy
# ---------------------------------------------------------------------------------------
def _int_degree(l):
    li = int(round(float(l)))
    if not np.isclose(float(l), li, atol=1e-9, rtol=0) or li < 0:
        raise ValueError('integer degree l >= 0 only (got %r): the non-integer-degree bases are out of scope' % (l,))
    return li


def _sph_jn(l, z, deriv=False):
    from scipy import special
    return special.spherical_jn(l, np.asarray(z, dtype=np.float64), derivative=bool(deriv))


def _sph_yn(l, z, deriv=False):
    """y_l clipped from below at -1e50, as the reference clips it wherever it divides or adds"""
    from scipy import special
    with np.errstate(all='ignore'):
        return np.clip(special.spherical_yn(l, np.asarray(z, dtype=np.float64), derivative=bool(deriv)), -1e50, np.inf)


def sph_bessel_kln(l, r_min, r_max, kmax=0.5, dk_factor=0.5, decimate=False, bc_type=2, add_kzero=False):
    """
    Radial wavenumbers k_ln [1/Mpc] of degree l that meet the boundary condition on a ball (r_min ~ 0) or a shell
    [r_min, r_max] (sph_harm.py:1171-1241): bc_type 1 (Dirichlet, the function vanishes at the edges) or 2 (Neumann, its
    derivative does); bc_type 3 (potential) is not built.  The condition is sampled on the reference's grid (from
    kmin = 1e-4 in steps of kmin * dk_factor up to kmax) and each sign change refined with utils.get_zeros.
    decimate keeps every other root; add_kzero prepends k = 0 for l = 0.
    """
    if bc_type == 3:
        raise NotImplementedError('bc_type=3 (potential boundary condition) is not built')
    if bc_type not in (1, 2):
        raise ValueError('bc_type must be 1 or 2')
    li = _int_degree(l)
    kmin = 1e-4
    dk = kmin * dk_factor
    ks = np.linspace(kmin, kmax, int((kmax - kmin) // dk) + 1)
    d = bc_type == 2
    if np.isclose(r_min, 0):
        y = _sph_jn(li, ks * r_max, d)
    else:
        y = _sph_jn(li, ks * r_min, d) * _sph_yn(li, ks * r_max, d) - _sph_jn(li, ks * r_max, d) * _sph_yn(li, ks * r_min, d)
    k = utils.get_zeros(ks, y)
    if decimate:
        k = k[::2]
    if add_kzero and li == 0:
        k = [0.0] + list(k)
    return np.asarray(k, dtype=np.float64)


def sph_bessel_func(l, k, r, method='shell', bc_type=2, r_crit=None, renorm=False, device=None, dtype=None):
    """
    Radial basis g_l(k_n r) = j_l(k_n r) + A_ln y_l(k_n r), (Nk, Nr) (sph_harm.py:1087-1168).  method 'ball': A = 0;
    'shell': A_ln = -j_l(k r_crit) / y_l(k r_crit) (bc_type 1) or the same ratio of derivatives (bc_type 2) at the edge
    r_crit, for k > 0.  y_l is clipped at -1e50.  Integer l only (scipy.special.spherical_jn / spherical_yn).
    renorm scales each row so that sum_r r^2 |g|^2 = pi / 2 / max(k, 1e-4)^2.  Evaluated in float64, returned as `dtype`.
    """
    if bc_type == 3:
        raise NotImplementedError('bc_type=3 (potential boundary condition) is not built')
    if method not in ('ball', 'shell'):
        raise ValueError("didn't recognize method {}".format(method))
    if method == 'shell' and r_crit is None:
        raise ValueError("method='shell' needs r_crit")
    li = _int_degree(l)
    k = np.atleast_1d(np.asarray(utils.tensor2numpy(k), dtype=np.float64))
    r = np.atleast_1d(np.asarray(utils.tensor2numpy(r), dtype=np.float64))
    kr = k[:, None] * r[None, :]
    g = _sph_jn(li, kr).reshape(len(k), len(r))
    if method == 'shell':
        pos = k > 0
        if pos.any():
            d = bc_type == 2
            A = -_sph_jn(li, k[pos] * r_crit, d) / _sph_yn(li, k[pos] * r_crit, d)
            g[pos] += A[:, None] * _sph_yn(li, kr[pos])
    if renorm:
        g *= np.sqrt(np.pi / 2 * k.clip(1e-4) ** -2.0 / np.sum(r ** 2 * np.abs(g) ** 2, axis=1))[:, None]
    return torch.as_tensor(g, device=device).to(dtype if dtype is not None else _float())


def gen_bessel2freq(l, r, kbins=None, Nproc=None, Ntask=10, device=None, dtype=None, method='shell', bc_type=2,
                    renorm=True, r_crit=None, use_pathos=False, **kln_kwargs):
    """
    Transform matrices sqrt(2/pi) r^2 max(k, 1e-4) g_l(k r) from radial wavenumber to line-of-sight distance, one per
    unique degree of l (sph_harm.py:955-1084).  Returns (gln, kln): dicts keyed by degree (in ascending order) of
    (Nk, Nr) tensors and of the k_ln arrays.  kbins: precomputed k_ln per degree; otherwise kln_kwargs (r_min, r_max and
    the keywords of sph_bessel_kln) give them.  renorm divides every row by its 2-norm (clipped at 1e-20).
    Nproc, Ntask and use_pathos (the reference's multiprocessing over degrees) are accepted and IGNORED: the scipy
    evaluation takes a fraction of a second per degree.  Evaluated in float64 whatever the default dtype, then cast.
    """
    r = np.atleast_1d(np.asarray(utils.tensor2numpy(r), dtype=np.float64))
    dtype = dtype if dtype is not None else _float()
    kw = copy.deepcopy(kln_kwargs)
    if kbins is None:
        r_min, r_max = kw.pop('r_min'), kw.pop('r_max')
    gln, kln = {}, {}
    for ll in np.unique(utils.tensor2numpy(l)):
        k = sph_bessel_kln(ll, r_min, r_max, bc_type=bc_type, **kw) if kbins is None else kbins[ll]
        k64 = np.atleast_1d(np.asarray(utils.tensor2numpy(k), dtype=np.float64))
        gl = sph_bessel_func(ll, k64, r, method=method, bc_type=bc_type, r_crit=r_crit, dtype=torch.float64).numpy()
        G = np.sqrt(2 / np.pi) * r ** 2 * k64[:, None].clip(1e-4) * gl
        if renorm:
            G = G / np.sqrt(np.sum(np.abs(G) ** 2, axis=1, keepdims=True).clip(1e-40))
        gln[ll] = torch.as_tensor(G, device=device).to(dtype)
        kln[ll] = k
    return gln, kln


class SFBModel:
    """
    Radial step of the spherical Fourier-Bessel transform, a_lm(r) = sum_n g_l(k_ln r) t_lmn (sph_harm.py:1851-2066):
    params (..., Nlmn) -> (..., Nr, Nlm).  The Nlmn axis is the concatenation, in the key order of `gln`, of per-degree
    blocks laid out [Nk][Nl] (k slow, column fast); the output columns of a degree are where `l` equals its key; columns
    whose degree has no key are 0.  All degrees run in ONE HIP launch (ops.sfb_radial) and one more backwards, instead
    of the reference's Python loop of per-degree matmuls.  Complex params give a complex output, real params a real one.
    The matrices are real: a complex-typed gln (which the reference needs, real @ complex raises in torch) is accepted
    when its imaginary part is 0 and stored once on the device as one packed real buffer in the parameters' precision.
    There is no CPU path.
    """
    def __init__(self, LM=None):
        self.LM = LM

    def setup_gln(self, l, gln=None, kln=None, out_dtype=None, r=None, m=None, **gln_kwargs):
        """
        l (Nlm,): degree of every output column; gln / kln: dicts from gen_bessel2freq (generated from r and gln_kwargs
        if gln is None; kln then serves as kbins); m (Nlm,), optional, fills m_arr.  Sets params_idx / alm_idx /
        alm_shape (per key), k_arr / l_arr / m_arr (per element of the Nlmn axis, in the reference's order), Nlmn, Nr,
        Nlm, out_dtype, device.
        """
        if gln is None:
            gln, kln = gen_bessel2freq(l, r, kbins=kln, dtype=out_dtype, **gln_kwargs)
        for key, G in gln.items():
            G = torch.as_tensor(G)
            if G.is_complex() and bool((G.imag != 0).any()):
                raise ValueError('gln[%r] has a non-zero imaginary part: the radial basis is real' % (key,))
        self.gln, self.kln, self.l, self.m = gln, kln, l, m
        l_np = np.asarray(utils.tensor2numpy(l))
        self.params_idx, self.alm_idx, self.alm_shape = {}, {}, {}
        k_arr, l_arr, m_arr = [], [], []
        n0 = 0
        for key, G in gln.items():
            Nk = len(G)
            idx = np.where(np.isclose(l_np, key, atol=1e-6, rtol=1e-10))[0]
            Nl = len(idx)
            self.params_idx[key] = slice(n0, n0 + Nk * Nl)
            self.alm_idx[key] = utils._list2slice(list(idx))
            self.alm_shape[key] = (G.shape[1], Nl)
            k_arr.extend(list(kln[key]) * Nl)
            l_arr.extend([key] * (Nk * Nl))
            if m is not None:
                m_arr.extend(mm for mm in np.asarray(m)[idx] for _ in range(Nk))
            n0 += Nk * Nl
        self.Nlmn = n0
        self.k_arr, self.l_arr, self.m_arr = np.asarray(k_arr), np.asarray(l_arr), np.asarray(m_arr)
        first = torch.as_tensor(next(iter(gln.values())))
        self.Nr = first.shape[1]
        self.Nlm = len(l_np)
        self.out_dtype = out_dtype if out_dtype is not None else _cfloat()
        self.device = first.device
        self._drop_plans()

    def _drop_plans(self):
        self.__dict__.pop('_plans', None)

    def __getstate__(self):
        # pickle / deepcopy: the packed device buffer and the int32 tables are derived from gln; the copy packs again on
        # first use (as AlmModel drops its conversion caches)
        state = dict(self.__dict__)
        state.pop('_plans', None)
        return state

    def _col_lists(self):
        return [np.arange(self.Nlm)[self.alm_idx[key]] if isinstance(self.alm_idx[key], slice)
                else np.asarray(self.alm_idx[key], dtype=np.int64) for key in self.gln]

    def _make_plan(self, gln, dtype, device):
        mats = []
        for key, G in gln.items():
            G = torch.as_tensor(G)
            if G.is_complex():
                if bool((G.imag != 0).any()):
                    raise ValueError('gln[%r] has a non-zero imaginary part: the radial basis is real' % (key,))
                G = G.real
            mats.append(G)
        return ops.SFBPlan(mats, self._col_lists(), self.Nr, self.Nlm, dtype, device)

    def _plan(self, dtype, device):
        plans = self.__dict__.setdefault('_plans', {})
        key = (dtype, str(device))
        if key not in plans:
            plans[key] = self._make_plan(self.gln, dtype, device)
        return plans[key]

    def __call__(self, params, **kwargs):
        return self.forward_gln(params, **kwargs)

    def forward_gln(self, params, gln=None):
        """
        params (..., Nlmn) -> (..., Nr, Nlm).  gln: use these matrices instead of self.gln (same keys in the same order,
        same shapes; packed for this call only).
        """
        if self.LM is not None:
            params = self.LM(params)
        if not params.is_cuda:
            raise RuntimeError('SFBModel.forward_gln needs GPU tensors (no CPU path)')
        rdt = params.real.dtype if params.is_complex() else params.dtype
        if gln is None:
            plan = self._plan(rdt, params.device)
        else:
            if list(gln.keys()) != list(self.gln.keys()):
                raise ValueError('gln keys differ from those of setup_gln')
            plan = self._make_plan(gln, rdt, params.device)
            want = [(len(self.gln[key]), self.alm_shape[key][1]) for key in self.gln]
            if plan.shapes != want:
                raise ValueError('gln shapes differ from those of setup_gln')
        return ops.sfb_radial(params, plan)

    def push(self, device):
        """move gln to a device, or re-type it (a dtype): the packed tables are rebuilt on the next call"""
        for key in self.gln:
            self.gln[key] = utils.push(torch.as_tensor(self.gln[key]), device)
        if self.LM is not None:
            self.LM.push(device)
        if isinstance(device, torch.dtype):
            self.out_dtype = device
        else:
            self.device = device
        self._drop_plans()

    def make_closure(self, params, loss_fn, target, real=False):
        """closure for an optimiser: zero the gradient, loss_fn(forward_gln(params), target) [real parts if `real`],
        backward, return the loss (sph_harm.py:2032-2066)"""
        def closure(params=params, loss_fn=loss_fn, target=target, real=real):
            if params.grad is not None:
                params.grad.zero_()
            out = self.forward_gln(params)
            tgt = target
            if real:
                out, tgt = out.real, target.real
            loss = loss_fn(out, tgt)
            loss.backward()
            return loss
        return closure


def sfb_binning(params, k_arr, kbins, var=None, wgts=None, l_arr=None, lbins=None):
    """
    Weighted average of a t_lmn tensor (..., Nlmn) into k bins (1-D) or (k, l) bins (2-D, when lbins is given), bins
    given by their centres (sph_harm.py:2069-2145).  Returns (binned params, binned variance).  As in the reference, an
    element belongs to bin i when np.digitize against the upper edges (centre + half the spacing to the next) gives i,
    the 1-D branch normalises the weights of a bin by their total before summing, the 2-D branch divides the sums by
    the total (variance: by its square) afterwards; empty bins give 0.
    """
    def edges(centres):
        centres = np.asarray(centres, dtype=np.float64)
        step = np.diff(centres)
        return centres + np.concatenate([step, step[-1:]]) / 2

    kind = np.digitize(k_arr, edges(kbins))
    Nk = len(kbins)
    if var is None:
        var = torch.ones_like(params)
    if wgts is None:
        wgts = torch.ones_like(params, dtype=_float())
    if lbins is None:
        out = torch.zeros(params.shape[:-1] + (Nk,), dtype=params.dtype, device=params.device)
        vout = torch.zeros_like(out)
        for i in range(Nk):
            sel = np.where(kind == i)[0]
            w = wgts[..., sel]
            w /= torch.sum(w).clip(1e-40)          # `w` is a copy (index-array selection): wgts itself is untouched
            out[..., i] = torch.sum(params[..., sel] * w, dim=-1)
            vout[..., i] = torch.sum(var[..., sel] * w ** 2, dim=-1)
        return out, vout
    lind = np.digitize(l_arr, edges(lbins))
    Nl = len(lbins)
    out = torch.zeros(params.shape[:-1] + (Nk, Nl), dtype=params.dtype, device=params.device)
    vout = torch.zeros_like(out)
    for i in range(Nk):
        for j in range(Nl):
            sel = np.where((kind == i) & (lind == j))[0]
            w = wgts[..., sel]
            tot = torch.sum(w).clip(1e-40)
            out[..., i, j] = torch.sum(params[..., sel] * w, dim=-1) / tot
            vout[..., i, j] = torch.sum(var[..., sel] * w ** 2, dim=-1) / tot ** 2
    return out, vout
