"""
Visibility filtering: the reference's filt.py restated on one HIP kernel.

`MatFilter`, `GPFilter`, `LstSqFilter` apply y = G x (or the residual x - G x, or an in-painting of the `input_idx` samples)
along one axis of a tensor or of a `dataset.VisData`; `WedgeFilter` applies a different member filter to each group of
baselines.  Signatures and attribute names follow the reference (filt.py:11-397); the covariance builders
(filt.py:404-651) and `invert_matrix` (linalg.py:365-478) are host-side set-up in torch.

Every application is ONE launch of `rime_filt_apply` (ops.filt_apply) and one more backwards: WedgeFilter maps each
baseline to the index of its filter, stacks the members' G and runs all groups together, where the reference loops over
the groups with a gather, a complex einsum and a scatter each (filt.py:382-397).  The data must be on the GPU; there is
no CPU path.  No gradient flows to G.

Left out: `linalg.least_squares`, `VisData.set`, filtering of CalData / MapData beyond their plain tensor.
"""
import numpy as np
import torch

from . import utils, dataset, ops


class BaseFilter(utils.Module):
    """Base class of the 1-D filters of tensors and VisData (filt.py:11-34)"""
    def __init__(self, dim=0, name=None, attrs=[]):
        super().__init__(name=name)
        self.dim = dim
        self.attrs = attrs
        self.device = None

    def push(self, device):
        """move the tensors named in self.attrs to a device, or re-type them (a dtype); plans are rebuilt on the next call"""
        if not isinstance(device, torch.dtype):
            self.device = device
        for attr in self.attrs:
            if isinstance(getattr(self, attr, None), torch.Tensor):
                setattr(self, attr, utils.push(getattr(self, attr), device))
        self._drop_plans()

    def _drop_plans(self):
        self.__dict__.pop('_plans', None)

    def __getstate__(self):
        # pickle / deepcopy: the packed device buffers and tile lists are derived from G; the copy packs again on first use
        state = dict(self.__dict__)
        state.pop('_plans', None)
        return state


class MatFilter(BaseFilter):
    """
    y_filt = G @ y along `dim`; with residual=True the output is y - G @ y; with input_idx only those samples of the
    input are replaced (filt.py:37-188).  G (N_pred_samples, N_data_samples), real or complex.
    """
    def __init__(self, G=None, dim=-1, dtype=None, device=None, residual=False, input_idx=None, inplace=False, name=None,
                 attrs=None):
        _attrs = attrs
        attrs = ['G', 'input_idx']
        if _attrs is not None:
            attrs += _attrs
        super().__init__(dim=dim, name=name, attrs=attrs)
        self.G = torch.as_tensor(G, device=device) if G is not None else G
        self.dtype = dtype
        self.residual = residual
        self.input_idx = input_idx
        self.inplace = inplace

    def setup_filter(self, G=None):
        """set the filter matrix (the reference's version names an undefined `device`, filt.py:87)"""
        self.G = torch.as_tensor(G, device=self.device) if G is not None else self.G
        self._drop_plans()

    def _indexed_G(self):
        G = self.G
        if getattr(self, '_idx', None) is not None:
            G = G[self._rowidx, self._idx]
        return G

    def _plan(self, kind, x):
        """FiltPlan of `predict` (plain G x) or `forward` (with residual / input_idx) in the precision and on the device of x"""
        G = self._indexed_G()
        if G is None:
            raise ValueError('%s has no filter matrix G' % self.name)
        rdt = x.real.dtype if x.is_complex() else x.dtype
        idx = self.input_idx if kind == 'forward' else None
        key = (kind, rdt, str(x.device), id(G), G._version, bool(self.residual), id(idx), getattr(idx, '_version', None))
        plans = self.__dict__.setdefault('_plans', {})
        if key not in plans:
            plans.clear()
            plans[key] = (ops.FiltPlan(G, residual=self.residual if kind == 'forward' else False, input_idx=idx, dtype=rdt,
                                       device=x.device), G, idx)        # G, idx kept alive: their ids are part of the key
        return plans[key][0]

    def predict(self, y, **kwargs):
        """y_filt = G @ y along self.dim; a tensor gives a tensor, a dataset a copy with its data replaced"""
        if isinstance(y, dataset.TensorData):
            out = y.copy()
            out.data = self.predict(out.data)
            return out
        return ops.filt_apply(y, self._plan('predict', y), dim=self.dim)

    def forward(self, y, **kwargs):
        """filter the input: G y, y - G y (residual), or y with its input_idx samples replaced by either"""
        if isinstance(y, np.ndarray):
            y = torch.as_tensor(y)
        elif isinstance(y, dataset.TensorData):
            out = y.copy(copydata=False, copymeta=False)
            out.data = self.forward(y.data, **kwargs)
            return out
        out = ops.filt_apply(y, self._plan('forward', y), dim=self.dim)
        if self.inplace and out.shape == y.shape and out.dtype == y.dtype:
            # the kernel reads every sample of a line for every output: it cannot write over its input, so in place is one
            # copy back (a filter whose output has another length returns a new tensor, as in the reference)
            y.copy_(out)
            return y
        return out

    def set_G_idx(self, idx=None, rowidx=None):
        """index G before applying it: idx picks rows and columns, or columns only when rowidx picks the rows"""
        if idx is not None and not isinstance(idx, slice):
            idx = torch.atleast_2d(torch.as_tensor(idx))
        self._idx = idx
        rowidx = rowidx if rowidx is not None else idx
        if rowidx is not None and not isinstance(rowidx, slice):
            rowidx = torch.atleast_2d(torch.as_tensor(rowidx)).T
        self._rowidx = rowidx
        self._drop_plans()


class GPFilter(MatFilter):
    """
    Gaussian-process (Wiener) filter: G = C_signal^pred [C_signal + C_noise]^-1, and the posterior variance
    V = Cs_pred - Cs C^-1 Cs^H (filt.py:191-314).
    """
    def __init__(self, Cs, Cn, Cs_cross=None, Cs_pred=None, dim=-1, dtype=None, device=None, residual=False, input_idx=None,
                 inplace=False, name=None, inv='pinv', hermitian=True, rcond=1e-15, eps=None):
        attrs = ['Cs', 'Cn', 'C', 'C_inv', 'G', 'V', 'input_idx']
        super().__init__(dim=dim, name=name, attrs=attrs, input_idx=input_idx, inplace=inplace)
        self.Cs = torch.as_tensor(Cs, device=device)
        self.Cn = torch.as_tensor(Cn, device=device)
        self.Cs_pred = torch.as_tensor(Cs_pred, device=device) if Cs_pred is not None else Cs_pred
        self.Cs_cross = torch.as_tensor(Cs_cross, device=device) if Cs_cross is not None else Cs_cross
        self.dtype = dtype
        self.residual = residual
        self.rcond = rcond
        self.hermitian = hermitian
        self.eps = eps
        self.inv = inv
        self.setup_filter()

    def setup_filter(self, Cs=None, Cn=None, Cs_pred=None, Cs_cross=None, inv=None, hermitian=None, rcond=None, eps=None):
        """C = Cs + Cn, C_inv = invert_matrix(C, ...), then set_GV(); arguments replace the stored ones"""
        self.Cs = self.Cs if Cs is None else Cs
        self.Cn = self.Cn if Cn is None else Cn
        self.Cs_pred = self.Cs_pred if Cs_pred is None else Cs_pred
        self.Cs_cross = self.Cs_cross if Cs_cross is None else Cs_cross
        self.C = self.Cs + self.Cn
        self.inv = self.inv if inv is None else inv
        self.hermitian = self.hermitian if hermitian is None else hermitian
        self.rcond = self.rcond if rcond is None else rcond
        self.eps = self.eps if eps is None else eps
        self.C_inv = invert_matrix(self.C, inv=self.inv, hermitian=self.hermitian, rcond=self.rcond, eps=self.eps)
        cast = lambda t: t if t is None else t.to(dtype=self.dtype, device=self.device)
        self.C_inv, self.Cs = cast(self.C_inv), cast(self.Cs)
        self.Cs_pred, self.Cs_cross = cast(self.Cs_pred), cast(self.Cs_cross)
        self.set_GV()

    def set_GV(self):
        """G = Cs C_inv and V = Cs_pred - Cs C_inv Cs^H from self.Cs (or Cs_cross), self.Cs_pred and self.C_inv"""
        Cs = self.Cs if self.Cs_cross is None else self.Cs_cross
        Cs_pred = self.Cs if self.Cs_pred is None else self.Cs_pred
        self.G = Cs @ self.C_inv
        self.V = Cs_pred - Cs @ self.C_inv @ Cs.T.conj()
        self._drop_plans()


class LstSqFilter(MatFilter):
    """a least-squares filter: a MatFilter whose default is the residual (filt.py:317-349)"""
    def __init__(self, G, dim=-1, device=None, dtype=None, residual=True, name=None):
        super().__init__(dim=dim, name=name, attrs=['G'])
        self.G = torch.as_tensor(G, device=device, dtype=dtype)
        self.device = device
        self.dtype = dtype
        self.residual = residual

    def setup_filter(self, G=None):
        self.G = torch.as_tensor(G, device=self.device, dtype=self.dtype) if G is not None else self.G
        self._drop_plans()


class WedgeFilter(utils.Module):
    """
    A baseline-dependent frequency filter (a wedge filter): filters[i] is applied to the baselines filt2bls[i], baselines
    in no group pass through unchanged (filt.py:352-401).  All groups run in ONE kernel launch, so the members must agree
    on the shape of G, on residual, on input_idx and filter the last axis; members with real and complex G are promoted
    to complex.  Input: a VisData (its own baselines are used) or a tensor (..., Nbl, Ntimes, Nfreqs) with `bls` given.
    """
    def __init__(self, filters, filt2bls, bls=None, inplace=False, name=None):
        super().__init__(name=name)
        self.filters = filters
        self.filt2bls = filt2bls
        self.inplace = inplace
        self.bls = bls
        self._bls2idx = {}
        if bls is not None:
            where = {tuple(bl): k for k, bl in reversed(list(enumerate(bls)))}
            for i, _bls in filt2bls.items():
                self._bls2idx[i] = [where[tuple(bl)] for bl in _bls]

    def _drop_plans(self):
        self.__dict__.pop('_plans', None)

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_plans', None)
        return state

    def _members(self):
        """the filters named by filt2bls, checked against each other; returns (keys, residual, input_idx)"""
        keys = sorted(self.filt2bls.keys())
        if not keys:
            raise ValueError('WedgeFilter without a filter group')
        first = self.filters[keys[0]]
        as_np = lambda t: None if t is None else np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t)
        for k in keys:
            f = self.filters[k]
            if getattr(f, 'G', None) is None:
                raise ValueError('filter %d has no matrix G' % k)
            if f.dim != -1:
                raise ValueError('filter %d filters dim %d: a WedgeFilter runs along the last axis (dim = -1)' % (k, f.dim))
            if f._indexed_G().shape != first._indexed_G().shape:
                raise ValueError('filters %d and %d differ in the shape of G: %s and %s' % (
                    keys[0], k, tuple(first._indexed_G().shape), tuple(f._indexed_G().shape)))
            if bool(f.residual) != bool(first.residual):
                raise ValueError('filters %d and %d differ in residual: %s and %s' % (keys[0], k, first.residual, f.residual))
            a, b = as_np(first.input_idx), as_np(f.input_idx)
            if (a is None) != (b is None) or (a is not None and (a.shape != b.shape or (a != b).any())):
                raise ValueError('filters %d and %d differ in input_idx' % (keys[0], k))
        return keys, bool(first.residual), first.input_idx

    def _bl2filt(self, bls):
        """filter slot (position in the stacked G) of every baseline of `bls`, -1 for a baseline in no group"""
        keys = sorted(self.filt2bls.keys())
        slot = {}
        for s, k in enumerate(keys):
            for bl in self.filt2bls[k]:
                bl = tuple(int(a) for a in bl)
                if bl in slot and slot[bl] != s:
                    raise ValueError('baseline %s belongs to the groups of filters %d and %d' % (bl, keys[slot[bl]], k))
                slot[bl] = s
        return tuple(slot.get(tuple(int(a) for a in bl), -1) for bl in bls)

    def _plan(self, x):
        rdt = x.real.dtype if x.is_complex() else x.dtype
        keys, residual, idx = self._members()
        Gs = [self.filters[k]._indexed_G() for k in keys]
        key = (rdt, str(x.device)) + tuple((id(G), G._version) for G in Gs)
        plans = self.__dict__.setdefault('_plans', {})
        if key not in plans:
            plans.clear()
            # mixed real and complex members ride the complex kernel; the plan casts to the precision of the data
            st = torch.complex128 if any(G.is_complex() for G in Gs) else torch.float64
            stack = torch.stack([G.detach().to(device=x.device, dtype=st) for G in Gs])
            plans[key] = (ops.FiltPlan(stack, residual=residual, input_idx=idx, dtype=rdt, device=x.device), Gs)
        return plans[key][0]

    def forward(self, vd, **kwargs):
        if isinstance(vd, dataset.VisData):
            out = vd.copy(copydata=False, copymeta=False)
            out.data = self._apply(vd.data, self._bl2filt(vd.bls), False)
            return out
        if self.bls is None:
            raise ValueError('WedgeFilter on a tensor needs the baselines of its third-last axis: pass bls')
        return self._apply(vd, self._bl2filt(self.bls), self.inplace)

    def _apply(self, x, b2f, inplace):
        if x.ndim < 3 or x.shape[-3] != len(b2f):
            raise ValueError('data of shape %s, expected (..., %d baselines, Ntimes, Nfreqs)' % (tuple(x.shape), len(b2f)))
        out = ops.filt_apply(x, self._plan(x), dim=-1, layout=(x.shape[-3], x.shape[-2], b2f))
        if inplace and out.shape == x.shape and out.dtype == x.dtype:
            x.copy_(out)
            return x
        return out

    def push(self, device):
        for filt in self.filters:
            filt.push(device)
        self._drop_plans()


# ---------------------------------------------------------------------------------------
# matrix inversion (linalg.py:365-478)
def cholesky_inverse(A, check_errors=True):
    """inverse of a positive-definite (M, M) matrix from its Cholesky factor L; returns (Ainv, L)"""
    if A.ndim == 1:
        return 1 / A, torch.sqrt(A)
    L = torch.linalg.cholesky_ex(A, check_errors=check_errors).L
    I = torch.eye(len(L), dtype=L.dtype, device=L.device)
    Linv = torch.linalg.solve_triangular(L, I, upper=False)
    return Linv.T.conj() @ Linv, L


def invert_matrix(A, inv='pinv', rcond=1e-15, hermitian=False, eps=None, driver=None):
    """
    Invert A over its last two dimensions (1 / A for a vector).  inv: 'inv' (torch.linalg.inv), 'pinv' (rcond, hermitian),
    'chol' (Cholesky inverse), 'lstsq' (rcond, driver), 'diag' (the diagonal only).  eps is added to the diagonal of A
    first, in place, as in the reference.
    """
    if inv == 'diag' or A.ndim == 1:
        if A.ndim == 1:
            return 1.0 / A
        return torch.diag(1.0 / torch.diag(A))

    def inverse(mat):
        if eps is not None:
            mat.diagonal().add_(eps)
        if inv == 'inv':
            return torch.linalg.inv(mat)
        elif inv == 'pinv':
            return torch.linalg.pinv(mat, rcond=rcond, hermitian=hermitian)
        elif inv == 'chol':
            return cholesky_inverse(mat)[0]
        elif inv == 'lstsq':
            return torch.linalg.lstsq(mat, torch.eye(len(mat), dtype=mat.dtype, device=mat.device), rcond=rcond,
                                      driver=driver).solution
        raise NameError("didn't recognize inv='{}'".format(inv))

    def recursive_inv(A, iA):
        if A.ndim > 2:
            for i in range(A.shape[0]):
                recursive_inv(A[i], iA[i])
            return
        iA[:, :] = inverse(A)

    iA = torch.zeros_like(A)
    recursive_inv(A, iA)
    return iA


# ---------------------------------------------------------------------------------------
# covariance builders (filt.py:404-651)
def _finish(cov, dtype, device):
    cov = cov.to(device)
    if dtype is not None:
        cov = cov.to(dtype)
    return cov


def rbf_cov(x, ls, amp=1, x2=None, dtype=None, device=None):
    """Gaussian (RBF) covariance amp exp(-dx^2 / (2 ls^2)); x2 gives a non-square (len(x2), len(x)) matrix"""
    x = torch.atleast_2d(x)
    x2 = x if x2 is None else torch.atleast_2d(x2)
    return _finish(amp * torch.exp(-.5 * (x2.T - x)**2 / ls**2), dtype, device)


def exp_cov(x, ls, amp=1, x2=None, dtype=None, device=None):
    """exponential covariance amp exp(-|dx| / ls)"""
    x = torch.atleast_2d(x)
    x2 = x if x2 is None else torch.atleast_2d(x2)
    return _finish(amp * torch.exp(-torch.abs(x2.T - x) / ls), dtype, device)


def sinc_cov(x, ls, amp=1, x2=None, dtype=None, device=None):
    """sinc covariance amp sinc(dx / ls)"""
    x = torch.atleast_2d(x)
    x2 = x if x2 is None else torch.atleast_2d(x2)
    return _finish(amp * torch.sinc((x2.T - x) / ls), dtype, device)


def phasor_mat(x, shift, neg=True, x2=None, dtype=None, device=None):
    """complex phasor matrix exp(-+ 2 pi i dx shift), minus for neg=True"""
    x = torch.atleast_2d(x)
    x2 = x if x2 is None else torch.atleast_2d(x2)
    coeff = 2j * np.pi
    if neg:
        coeff *= -1
    return _finish(torch.exp(coeff * (x2.T - x) * shift), dtype, device)


def gauss_sinc_cov(x, gauss_ls, sinc_ls, x2=None, dtype=None, device=None, high_prec=True):
    """
    Gaussian-convolved sinc covariance (a top-hat truncated Gaussian in Fourier space; arXiv:1608.05854, appendix A2).
    high_prec: evaluate the complex error functions with mpmath, else with torch (NaN replaced by 0).
    """
    from scipy import special
    sinc_ls = sinc_ls / np.pi
    arg = gauss_ls / np.sqrt(2) / sinc_ls
    xc = x / gauss_ls / np.sqrt(2)
    x2c = xc if x2 is None else x2 / gauss_ls / np.sqrt(2)
    dists = (x2c[:, None] - xc[None, :])
    ud, ui = torch.unique(dists, return_inverse=True)
    if high_prec:
        import mpmath
        fn = lambda z: mpmath.exp(-z**2) * (mpmath.erf(arg + 1j*z) + mpmath.erf(arg - 1j*z)).real
        K = 0.5 * torch.as_tensor(np.asarray(np.frompyfunc(fn, 1, 1)(ud.numpy()), dtype=float))
        K /= special.erf(arg)
    else:
        K = (0.5 * torch.exp(-ud**2) / torch.special.erf(torch.as_tensor(arg))
             * (torch.special.erf(arg + 1j*ud) + torch.special.erf(arg - 1j*ud))).real
        K[torch.isnan(K)] = 0.0
    cov = K[ui]
    cov[torch.isclose(dists, torch.tensor(0., dtype=dists.dtype), atol=1e-7)] = 1.0
    if dtype is not None:
        cov = cov.to(dtype)
    if device is not None:
        cov = cov.to(device)
    return cov


def gen_cov_modes(cov, N=None, rcond=None, device=None, dtype=None):
    """eigenmodes of a hermitian covariance, largest first: the top N, or those with eigenvalue >= max * rcond;
    returns (A (M, N), all eigenvalues)"""
    assert N is None or rcond is None, "cannot provide both N and rcond"
    evals, A = torch.linalg.eigh(cov)
    A = A.flip([1])
    evals = evals.flip([0])
    if N is not None:
        A = A[:, :N]
    elif rcond is not None:
        A = A[:, evals >= evals.max() * rcond]
    A = A.to(device)
    if dtype is not None:
        A = A.to(dtype)
    return A, evals
