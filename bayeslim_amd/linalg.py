"""
The least-squares pieces of the reference's linalg.py that LinearModel.least_squares needs (linalg.py:404-478 invert_matrix,
:481-760 least_squares), same names, argument meaning and results.

least_squares solves y = A x along one axis of y.  In mode='matrix' the product A^H y -- the only pass over the data -- is ONE
launch of `rime_lm_apply` in its transpose direction (ops.lm_apply(adjoint=True)); the small (Nfeatures, Nfeatures) normal
matrix, its inverse D and the application of D stay torch.  Covered: norm None / 'inv' / 'pinv' / 'chol' / 'diag', eps, rcond,
hermitian, a passed D, Ninv as a 1-D diagonal (or of y's shape for norm='diag' and norm=None), and mode='lstsq' through
torch.linalg.lstsq.  pretran, preconj, a full-matrix Ninv (Ndiag=False) and a batched A raise NotImplementedError.
"""
import torch

from . import ops
from .filt import invert_matrix  # noqa: F401  (the package's one implementation: 'inv', 'pinv', 'chol', 'lstsq', 'diag')


def _along(vec, ndim, dim):
    shape = [1] * ndim
    shape[dim] = -1
    return vec.reshape(shape)


def least_squares(A, y, dim=0, mode='matrix', norm='inv', pinv=True, eps=0, rcond=1e-15, hermitian=True, D=None,
                  preconj=False, pretran=False, driver=None, Ninv=None, Ndiag=True, plan=None):
    """
    Generalised least squares of y = A x along axis `dim` of y (linalg.py:481-760):

        xhat = D A^H N^-1 y,        D = (A^H N^-1 A + eps I)^-1

    A (Nsamples, Nfeatures), y (..., Nsamples, ...) of up to 8 axes.  mode='matrix': norm None (D = 1), 'inv' (with pinv=True,
    the default, the pseudo-inverse), 'pinv', 'chol' (Cholesky inverse) or 'diag' (the inverse of the diagonal of A^H N^-1 A, clipped at 1e-40); D, when
    passed, is used as it is.  Ninv: the inverse noise variance, 1-D along `dim`, or of y's shape for norm='diag' / None.
    mode='lstsq': torch.linalg.lstsq on sqrt(Ninv)-weighted A and y.  Returns (xhat, D); D is None in 'lstsq' mode.

    `plan` (an ops.LMPlan of A without idx / coeff) saves rebuilding the device tables of A^H on every call.  In 'matrix' mode y
    lives on the GPU (there is no CPU path).  Raises NotImplementedError for pretran, preconj, Ndiag=False and a batched A (A.ndim > 2).
    """
    assert y.ndim <= 8
    if pretran or preconj:
        raise NotImplementedError('least_squares(pretran / preconj): pass A as (Nsamples, Nfeatures), not conjugated')
    if Ninv is not None and not Ndiag:
        raise NotImplementedError('least_squares with a full-matrix Ninv (Ndiag=False); pass the diagonal of N^-1')
    if A.ndim != 2:
        raise NotImplementedError('least_squares with a batched A of %d axes: only a 2-D design matrix is served' % A.ndim)
    d = dim % y.ndim

    if mode == 'lstsq':
        if Ninv is not None:
            Ninv = torch.sqrt(Ninv)
            y = (_along(Ninv, y.ndim, d) if Ninv.ndim == 1 else Ninv) * y
            A = A * Ninv[:, None]
        if A.ndim < y.ndim:
            A = A.reshape(torch.Size([1] * (y.ndim - A.ndim)) + A.shape)
        if y.ndim > 1:
            y = y.moveaxis(d, -2)
        xhat = torch.linalg.lstsq(A, y, driver=driver).solution
        if y.ndim > 1:
            xhat = xhat.moveaxis(-2, d)
        return xhat, None
    assert mode == 'matrix'

    if Ninv is not None:
        if Ninv.ndim != 1 and norm not in ('diag', None):
            raise NotImplementedError("an Ninv of y's shape is served for norm='diag' and norm=None only")
        y = (_along(Ninv, y.ndim, d) if Ninv.ndim == 1 else Ninv) * y

    # A^H y: the one pass over the data
    if plan is None:
        plan = ops.LMPlan(A)
    xhat = ops.lm_apply(y, plan, dim=d, adjoint=True)

    if norm in ('inv', 'pinv', 'chol'):
        if D is None:
            Ah = A.conj().T
            Dinv = Ah @ A if Ninv is None else Ah @ (Ninv[:, None].to(A.dtype) * A)
            if torch.is_complex(Dinv):
                Dinv = Dinv.real
            if norm == 'inv' and pinv:
                norm = 'pinv'
            D = invert_matrix(Dinv, inv=norm, rcond=rcond, eps=eps, hermitian=hermitian)
        xhat = torch.movedim(torch.tensordot(xhat, D.to(device=xhat.device, dtype=xhat.dtype), dims=([d], [1])), -1, d)
    elif norm == 'diag':
        if D is None:
            if Ninv is None:
                Dinv = A.norm(dim=-2).pow(2)
            elif Ninv.ndim == 1:
                Dinv = (Ninv[:, None] * torch.abs(A) ** 2).sum(dim=-2)
            else:
                A2 = (torch.abs(A) ** 2).to(device=Ninv.device, dtype=Ninv.dtype)
                Dinv = torch.movedim(torch.tensordot(Ninv, A2, dims=([d], [0])), -1, d)
            if torch.is_complex(Dinv):
                Dinv = Dinv.real
            D = 1 / Dinv.clip(1e-40)
        Duse = D.to(xhat.device)
        if Duse.ndim == 1:
            Duse = _along(Duse, xhat.ndim, d)
        elif Duse.ndim != xhat.ndim:
            shape = [1] * xhat.ndim
            shape[d - Duse.ndim + 1:d + 1] = Duse.shape
            Duse = Duse.reshape(shape)
        xhat = Duse * xhat
    else:
        D = torch.ones(A.shape[-1])                            # no normalisation (any other norm, as in the reference)

    return xhat, D
