"""
Linear models y = A x (reference linear_model.py, whole file): LinearModel, MultiLM, DictLM and the design matrices
gen_linear_A / gen_poly_A / gen_fourier_A, with the reference's names, arguments, attributes and results.  They are what
goes into `freq_LM` / `time_LM` / `spat_LM` of the response classes (freq_mode='linear'):

    freq_LM = linear_model.LinearModel('poly', dim=-2, x=freqs, Ndeg=6, basis='legendre')
    R = sky_model.PixelSkyResponse(freqs, freq_mode='linear', freq_LM=freq_LM)

Every product runs as ONE launch of `rime_lm_apply` (ops.lm_apply; csrc/lm.hip) whatever the axis: the reference's chain
params * coeff -> index_select -> matmul / einsum -> .real (linear_model.py:121-169) reads its input once and writes its
output once, and the backward pass and the A^H y product of least_squares are the same kernel with A^H.  There is no CPU
path: parameters on the CPU raise, except with diag=True, which is an elementwise torch product as in the reference.
"""
import copy

import numpy as np
import torch

from . import utils, linalg, ops
from .utils import _float


class LinearModel:
    """
    A linear model y = A x along one axis of a parameter tensor (linear_model.py:15-259).
    """
    def __init__(self, linear_mode, dim=0, coeff=None, diag=False, idx=None, out_dtype=None, out_reshape=None,
                 out_shape=None, out_real=False, meta=None, **kwargs):
        """
        linear_mode : 'custom' (pass A=), 'poly' or 'fourier'; kwargs go to gen_linear_A
        dim : the axis of the parameter tensor that A contracts
        coeff : tensor multiplied into the parameters first.  A real vector along `dim` (1-D for the last axis, or all other
            axes of length 1) is fused into the kernel; any other shape is multiplied in torch before the launch
        diag : A is diagonal; only its diagonal is kept and forward() is an elementwise torch product ('custom' only)
        idx : index tensor applied along `dim` after coeff, (params * coeff)[idx]; fused into the kernel's loads
        out_dtype, out_reshape : cast / reshape of the result;  out_shape : the result's shape before out_reshape, which
            least_squares() needs to undo it;  out_real : return Re(A x) only (the kernel then computes nothing else)
        meta : dict kept as self.meta
        """
        self.linear_mode, self.dim, self.diag = linear_mode, dim, diag
        self.coeff, self.idx = coeff, idx
        self.out_dtype, self.out_reshape, self.out_shape, self.out_real = out_dtype, out_reshape, out_shape, out_real
        self.meta = {} if meta is None else meta
        self._D = None                                 # normalisation matrix kept by least_squares(cache_D=True)
        if linear_mode == 'poly' and kwargs.get('whiten', False):
            # pin the centre and the scale of the whitening to this x, so that generate_A() at other samples reuses them
            prep = {k: kwargs.get(k) for k in ('d0', 'x0', 'dx')}
            _, x0, dx = utils.prep_xarr(kwargs.get('x'), logx=kwargs.get('logx', False), whiten=True, **prep)
            for name, val in (('x0', x0), ('dx', dx)):
                if not kwargs.get(name, None):
                    kwargs[name] = val
        self.kwargs = kwargs
        self.A = gen_linear_A(linear_mode, **kwargs)
        self._A_ndim = self.A.ndim
        if diag and self._A_ndim == 2:
            self.A = torch.diag(self.A)
        self.device = self.A.device
        self.freqs = None
        if linear_mode == 'fourier':
            self.freqs = gen_fourier_A(kwargs.get('x'), Ndeg=kwargs.get('Ndeg'), fft_norm=kwargs.get('fft_norm', 'ortho'))[1]

    # ---- device-side state
    def _plan(self, use, A, idx=None, cvec=None):
        """
        The LMPlan of the model's own (A, idx, coeff vector) for one use ('fwd' or 'ls'), kept while it was built from these
        very tensors at their present versions (an in-place edit or a replaced tensor gets a new plan).
        """
        stamp = [(t, None if t is None else t._version) for t in (A, idx, cvec)]
        plans = self.__dict__.setdefault('_plans', {})
        held = plans.get(use)
        if held is None or any(a is not b or va != vb for (a, va), (b, vb) in zip(held[0], stamp)):
            held = plans[use] = (stamp, ops.LMPlan(A, idx=idx, coeff=cvec))
        return held[1]

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_plans', None)
        return state

    def __deepcopy__(self, memo):
        new = type(self).__new__(type(self))
        new.__dict__.update({k: copy.deepcopy(v, memo) for k, v in self.__getstate__().items()})
        return new

    @staticmethod
    def _coeff_vector(coeff, shape, d):
        """coeff as a 1-D vector along axis d of a tensor of `shape` if it is one (real, no gradient), else None"""
        if not isinstance(coeff, torch.Tensor) or coeff.is_complex() or coeff.requires_grad:
            return None
        if not (coeff.is_floating_point() and coeff.numel() == shape[d]):
            return None
        if coeff.ndim == 1:
            return coeff if d == len(shape) - 1 else None
        if coeff.ndim == len(shape) and coeff.shape[d] == shape[d]:
            return coeff.reshape(-1)
        return None

    def forward(self, params, A=None, coeff=None):
        """
        y = A (coeff * params)[idx] along self.dim, then out_dtype, out_real, out_reshape (linear_model.py:99-169).

        params : tensor of up to 8 axes, real or complex, on the GPU
        A : (Nsamples, Nfeatures) design matrix used instead of self.A ((Nsamples,) with diag=True)
        coeff : used instead of self.coeff

        Raises NotImplementedError for a batched A (A.ndim > 2: one design matrix per leading index, which the reference
        contracts with an einsum): the kernel applies one matrix.
        """
        own = A is None and coeff is None
        A = self.A if A is None else A
        coeff = self.coeff if coeff is None else coeff
        idx = getattr(self, 'idx', None)
        params = torch.as_tensor(params) if not isinstance(params, torch.Tensor) else params
        ndim = params.ndim

        if self.diag:
            # elementwise, as in the reference
            if coeff is not None:
                params = params * coeff
            if idx is not None:
                params = torch.index_select(params, self.dim, idx)
            if len(A) > 1:
                A = A.reshape([-1 if i == self.dim % ndim else 1 for i in range(ndim)])
            out = A * params
            if self.out_dtype is not None:
                out = out.to(self.out_dtype)
            if self.out_real:
                out = out.real
        else:
            if A.ndim > 2:
                raise NotImplementedError('LinearModel.forward with a batched A of shape %s: the HIP kernel applies one '
                                          '(Nsamples, Nfeatures) matrix; loop over the leading axes' % (tuple(A.shape),))
            assert ndim <= 8
            d = 0 if ndim == 1 else self.dim % ndim
            cvec = None
            if coeff is not None:
                cvec = self._coeff_vector(coeff, tuple(params.shape), d)
                if cvec is None:
                    params = params * coeff
            # an A or coeff passed for this call gets a plan of its own, which is not kept
            plan = self._plan('fwd', A, idx, cvec) if own else ops.LMPlan(A, idx=idx, coeff=cvec)
            out = ops.lm_apply(params, plan, dim=d, out_real=self.out_real)
            if self.out_dtype is not None:
                odt = self.out_dtype
                if not out.is_complex() and self.out_real and odt.is_complex:
                    odt = odt.to_real()
                out = out.to(odt)
            if self.out_real and out.is_complex():
                out = out.real

        if getattr(self, 'out_reshape', None) is not None:
            out = out.reshape(self.out_reshape)
        return out

    def __call__(self, params, A=None):
        return self.forward(params, A=A)

    def least_squares(self, y, out_shape=None, Ninv=None, cache_D=False, **kwargs):
        """
        Estimate the parameter tensor from y = A x (linear_model.py:174-214): y is cast to A's dtype, out_reshape is undone
        through out_shape (an Ninv of y's shape with it), then linalg.least_squares(A, y, dim=self.dim, Ninv=Ninv, D=self._D,
        **kwargs), whose A^H y product runs on the kernel.  cache_D keeps the normalisation matrix as self._D for later calls.
        idx and coeff play no part, as in the reference.
        """
        A, plan = self.A, None
        y = y if y.dtype == A.dtype else y.to(A.dtype)
        if self.diag:
            A = torch.diag(A if len(A) == y.shape[self.dim] else A.expand(y.shape[self.dim]))
        elif A.ndim == 2:
            plan = self._plan('ls', A)
        shape = self.out_shape if out_shape is None else out_shape
        if shape is not None:
            if Ninv is not None and Ninv.shape == y.shape:
                Ninv = Ninv.reshape(shape)
            y = y.reshape(shape)
        xhat, D = linalg.least_squares(A, y, dim=self.dim, Ninv=Ninv, D=self._D, plan=plan, **kwargs)
        if cache_D:
            self._D = D
        return xhat

    def generate_A(self, x, **interp1d_kwargs):
        """
        A design matrix at new sample values x (linear_model.py:216-246): 'custom' interpolates self.A along its samples
        (scipy interp1d with these kwargs), the other modes regenerate A from the stored set-up.
        """
        if self.linear_mode == 'custom':
            from scipy.interpolate import interp1d
            rows = interp1d(self.kwargs['x'], self.A.cpu().numpy(), axis=0, **interp1d_kwargs)(x)
            return torch.as_tensor(rows).to(self.device)
        return gen_linear_A(self.linear_mode, **dict(copy.deepcopy(self.kwargs), x=x)).to(self.device)

    def push(self, device):
        """move A, coeff and idx to a device, or A and coeff to a dtype; the kernel's tables are rebuilt on the next call"""
        self.A = utils.push(self.A, device)
        self.coeff = utils.push(self.coeff, device)
        if not isinstance(device, torch.dtype):
            self.device = device
            self.idx = utils.push(getattr(self, 'idx', None), device)
        self.__dict__.pop('_plans', None)


class MultiLM:
    """
    Several LinearModel objects applied in turn, each along its own axis of one tensor (linear_model.py:262-297);
    least_squares runs through them in the same order.
    """
    def __init__(self, LM):
        self.LM = LM

    def forward(self, params, **kwargs):
        for model in self.LM:
            params = model(params, **kwargs)
        return params

    __call__ = forward

    def least_squares(self, y, **kwargs):
        for model in self.LM:
            y = model.least_squares(y, **kwargs)
        return y

    def push(self, device):
        for model in self.LM:
            model.push(device)


class DictLM:
    """
    Linear models keyed by parameter name, e.g. 'rime.sky.eor.params' (linear_model.py:300-344); an unknown name is an error.
    """
    def __init__(self, LMs):
        self.LMs = LMs
        self.device = next(iter(LMs.values())).device

    def forward(self, name, params, **kwargs):
        assert name in self.LMs
        return self.LMs[name](params, **kwargs)

    __call__ = forward

    def least_squares(self, name, y, **kwargs):
        return self.LMs[name].least_squares(y, **kwargs)

    def push(self, device):
        for model in self.LMs.values():
            model.push(device)
        self.device = next(iter(self.LMs.values())).device


def gen_linear_A(linear_mode, A=None, x=None, d0=None, logx=False, whiten=True, x0=None, dx=None, Ndeg=None, basis='direct',
                 qr=False, device=None, dtype=None, fft_norm='ortho', **kwargs):
    """
    Design matrix (Nsamples, Nfeatures) of a linear mapping (linear_model.py:347-411).

    linear_mode : 'poly' (gen_poly_A: x, Ndeg, basis, d0, logx, whiten, x0, dx, qr), 'custom' (A as passed) or 'fourier'
        (gen_fourier_A: x, Ndeg, fft_norm)
    device, dtype : where and as what A is returned; dtype defaults to A's own when A is passed, else to utils._float().
        As in the reference, that default casts the complex matrix of 'fourier' to REAL (torch drops the imaginary part, with
        a warning): pass dtype=utils._cfloat() for the complex Fourier basis.
    """
    if linear_mode == 'poly':
        out = gen_poly_A(x, Ndeg, basis=basis, d0=d0, logx=logx, whiten=whiten, x0=x0, dx=dx, qr=qr)
    elif linear_mode == 'fourier':
        out = gen_fourier_A(x, Ndeg=Ndeg, device=device, fft_norm=fft_norm)[0]
    elif linear_mode == 'custom':
        assert A is not None
        out = torch.as_tensor(A)
    else:
        raise NameError("linear_mode {} not recognized".format(linear_mode))
    if dtype is None:
        dtype = utils._float() if A is None else A.dtype
    return torch.atleast_1d(out).to(dtype).to(device)


def gen_fourier_A(x, Ndeg=None, device=None, fft_norm='ortho'):
    """
    Complex Fourier-series matrix (Nsamples, Ndeg) over uniform samples x, and its frequencies (linear_model.py:414-447):
    the fftshifted DFT of the identity under `fft_norm`, cut to the Ndeg central modes when Ndeg is given.  Returns (A, freqs).
    """
    n = len(x)
    A = torch.fft.fftshift(torch.fft.fft(torch.eye(n), dim=-1, norm=fft_norm), dim=-1)
    freqs = torch.fft.fftshift(torch.fft.fftfreq(n, torch.as_tensor(x[1] - x[0])))
    if Ndeg is not None:
        lo = n // 2 - Ndeg // 2                          # the Ndeg central modes
        A, freqs = A[:, lo:lo + Ndeg], freqs[lo:lo + Ndeg]
    return A, freqs


def gen_poly_A(x, Ndeg, device=None, basis='direct', d0=None, logx=False, whiten=True, x0=None, dx=None, qr=False):
    """
    Polynomial design matrix (Nx, Ndeg), y = a_0 P_0(x) + a_1 P_1(x) + ... (linear_model.py:450-515).

    basis : 'direct' (x^i), 'legendre', 'chebyshevt', 'chebyshevu' or 'laguerre' (scipy.special, imported here)
    d0, logx, whiten, x0, dx : preparation of x, see utils.prep_xarr
    qr : re-orthogonalise the columns by a QR factorisation
    """
    x, _, _ = utils.prep_xarr(torch.as_tensor(x), d0=d0, logx=logx, whiten=whiten, x0=x0, dx=dx)
    x = x.detach().cpu().numpy()

    evaluate = {'direct': lambda i, t: t ** i}
    if basis in ('legendre', 'chebyshevt', 'chebyshevu', 'laguerre'):
        from scipy import special
        evaluate = {'legendre': special.eval_legendre, 'chebyshevt': special.eval_chebyt, 'chebyshevu': special.eval_chebyu,
                    'laguerre': special.eval_laguerre}
    if basis not in evaluate:
        raise NameError("didn't recognize basis {}".format(basis))
    A = np.stack([evaluate[basis](i, x) for i in range(Ndeg)], axis=1)
    if qr:
        A = np.linalg.qr(A)[0]
    return torch.as_tensor(A, dtype=_float(), device=device)
