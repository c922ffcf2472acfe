"""
The quasi-Newton optimisers of the reference's bfgs.py on HIP kernels: L-BFGS with its search direction on the fused kernels
of csrc/lbfgs.hip (LBFGS, two_loop_recursion, strong_wolfe, cubic_interpolate) for a starting inverse Hessian that is the
identity, a scalar, a diagonal or an hmat operator; dense BFGS on the two passes of csrc/bfgs.hip (BFGS, implicit_to_dense);
and the factored inverse Hessian that turns a run of either into a covariance estimate (FactoredInvHessian, factor_pairs,
factored_hvp, factored_lvp, lbfgs_approx_cov).

The two-loop recursion over m pairs (s_j, y_j) with H0 = gamma * diag(d) is a function of the inner products
SY[i, j] = s_i . y_j, YDY[i, j] = y_i . (d o y_j), Sv[i] = s_i . v and YDv[i] = y_i . (d o v) (the compact representation of
Byrd, Nocedal & Schnabel, Math. Prog. 63, 1994):

    alpha_i = rho_i (Sv_i - sum_{j > i} alpha_j SY[i, j])                                      i = m - 1 ... 0
    beta_i  = rho_i (gamma (YDv_i - sum_j alpha_j YDY[i, j]) + sum_{j < i} (alpha_j - beta_j) SY[j, i])      i = 0 ... m - 1
    r = gamma * d o (v - sum_j alpha_j y_j) + sum_j (alpha_j - beta_j) s_j

compact_coeffs() is that recurrence on the host in float64; rime_lbfgs_dots gives the inner products in one pass over the
history and rime_lbfgs_combine the last line in another.  LBFGS keeps SY and YDY: a new pair adds one row and one column, from
the same dots launch that serves the next direction.  The history is handed to the kernels as tables of row addresses (the
tensors the optimiser holds anyway), so nothing is copied when the ring wraps.

Complex parameters pass through the kernels as their interleaved real views: Re(s^H q) is the real dot product of the views,
and a real diagonal is repeated per component.  There is no CPU path.

With an hmat operator (hmat.BaseMat, hmat.HierMat) as H0 the product H0 q cannot be folded into the Gram quantities, so the
direction is the two half-recurrences around it, on the same kernels: rime_lbfgs_dots on v for s_j . v, first_loop() on the
host, rime_lbfgs_combine for q = v - sum_j a_j y_j, z = gamma * H0 q through the operator's plan (hmat.py), rime_lbfgs_dots on z
for y_j . z, second_loop() on the host and rime_lbfgs_combine for r = z + sum_j b_j s_j.  update_Hdiag keeps the operator as
it is and rescales gamma with the operator's diagonal as the metric of eqn 7.20 (the reference multiplies the scalar into the
operator in place; the product gamma * H0 is the same).

Dense BFGS (BFGS, implicit_to_dense) keeps the N x N inverse Hessian on the GPU and updates it in place on the kernels of
csrc/bfgs.hip.  The reference's update V^T H V + rho s s^T, V = I - rho y s^T, is the symmetric rank-two correction

    w = H y,  theta = y . w,  rho = 1 / (y . s):     H <- H - rho (s w^T + w s^T) + (rho^2 theta + rho) s s^T

so one pass reads H for a product (rime_bfgs_matvec) and one reads and writes it for the correction (rime_bfgs_rank2).
step() needs one product per iteration: H_k g_k = -p_k is known, so with u = H_k g_{k+1} the product w = H_k y_k = u + p_k costs
O(N), and the next direction follows from u, w, s:  H_{k+1} g_{k+1} = u - rho ((w . g) s + (s . g) w) + (rho^2 theta + rho) (s . g) s
with g = g_{k+1}.  H y stands for y^T H too: H0 must be symmetric (an H0 that is not, beyond rounding, is refused).

The factored form of Brodlie, Gourlay & Greenstadt (1973), H = L L^T with L = (I + u_m v_m^T) ... (I + u_1 v_1^T) L0
(factor_pairs, factored_lvp, factored_hvp, FactoredInvHessian), runs on the L-BFGS kernels: a chain of shells
vec <- vec + u_k (v_k . vec), k = 0 ... m - 1, is the recurrence c_k = v_k . vec0 + sum_{j < k} (v_k . u_j) c_j with the result
vec0 + sum_k c_k u_k: one rime_lbfgs_dots launch with the tables S = u, Y = v, forward_shell() on the host in float64, one
rime_lbfgs_combine launch.  The reversed chain of the transposed factor, vec <- vec + v_k (u_k . vec), k = m - 1 ... 0, is
reverse_shell() on the transposed Gram matrix.  FactoredInvHessian keeps the Gram matrix G[k, j] = v_k . u_j and the tables.
lbfgs_approx_cov gives the diagonal estimate per parameter group of an optim.LogProb as an hmat.DiagMat.

Out of scope: the ParamDict line search.
"""
import ctypes
import math
from collections import deque

import numpy as np
import torch

from . import _lib, hmat
from .ops import _require_cuda, _stream, _ptr

# elements of one work-group of rime_lbfgs_dots (256 lanes x 64 bytes): the unit of its first reduction stage
DOTS_SPAN = {torch.float32: 4096, torch.float64: 2048}


def compact_coeffs(SY, YDY, Sv, YDv, gamma, rho=None):
    """
    The two loops of the recursion on the Gram quantities of the module docstring, float64 on the host.

    SY, YDY : (m, m) array-likes;  Sv, YDv : (m,);  gamma : float;  rho : (m,) or None for 1 / diag(SY).
    Returns (a, b), float64 arrays of length m with r = gamma d o (v - sum a_j y_j) + sum b_j s_j.
    """
    SY, YDY = np.asarray(SY, dtype=np.float64), np.asarray(YDY, dtype=np.float64)
    Sv, YDv = np.asarray(Sv, dtype=np.float64), np.asarray(YDv, dtype=np.float64)
    m = len(Sv)
    rho = 1.0 / np.diagonal(SY) if rho is None else np.asarray([float(x) for x in rho], dtype=np.float64)
    gamma = float(gamma)
    alpha, b = np.zeros(m), np.zeros(m)
    for i in range(m - 1, -1, -1):
        alpha[i] = rho[i] * (Sv[i] - SY[i, i + 1:] @ alpha[i + 1:])
    t = gamma * (YDv - YDY @ alpha)
    for i in range(m):
        beta = rho[i] * (t[i] + b[:i] @ SY[:i, i])
        b[i] = alpha[i] - beta
    return alpha, b


def first_loop(SY, Sv, rho=None):
    """alpha of the first loop of the recursion: alpha_i = rho_i (Sv_i - sum_{j > i} alpha_j SY[i, j]), i = m - 1 ... 0; float64
    on the host.  q = v - sum_j alpha_j y_j is what the starting matrix is applied to."""
    SY, Sv = np.asarray(SY, dtype=np.float64), np.asarray(Sv, dtype=np.float64)
    m = len(Sv)
    rho = 1.0 / np.diagonal(SY) if rho is None else np.asarray([float(x) for x in rho], dtype=np.float64)
    alpha = np.zeros(m)
    for i in range(m - 1, -1, -1):
        alpha[i] = rho[i] * (Sv[i] - SY[i, i + 1:] @ alpha[i + 1:])
    return alpha


def second_loop(SY, Yz, alpha, rho=None):
    """b of the second loop for z = H0 q: beta_i = rho_i (Yz_i + sum_{j < i} b_j SY[j, i]), b_i = alpha_i - beta_i, i = 0 ... m - 1,
    with Yz_i = y_i . z; r = z + sum_j b_j s_j."""
    SY, Yz = np.asarray(SY, dtype=np.float64), np.asarray(Yz, dtype=np.float64)
    m = len(Yz)
    rho = 1.0 / np.diagonal(SY) if rho is None else np.asarray([float(x) for x in rho], dtype=np.float64)
    b = np.zeros(m)
    for i in range(m):
        b[i] = alpha[i] - rho[i] * (Yz[i] + b[:i] @ SY[:i, i])
    return b


def _is_operator(H0):
    return isinstance(H0, (hmat.BaseMat, hmat.HierMat))


def _operator_direction(hist, op, gamma, vec, SY, Sv, rho=None):
    """the direction with an hmat operator as the starting matrix (module docstring); hist holds the pairs, vec is the vector in
    the parameters' own dtype, Sv = s_j . v from a dots launch on its real view"""
    v = _real_view(vec)
    d, hist.d = hist.d, None                      # the plain inner products and combinations: no diagonal in the passes
    try:
        zero = np.zeros(len(Sv))
        alpha = first_loop(SY, Sv, rho)
        q = hist.combine(v, alpha, zero, 1.0)
        z = _real_view(hmat._apply(op, _shape_like(q, vec), scalar=None if gamma == 1.0 else gamma))
        b = second_loop(SY, hist.dots(z)[1], alpha, rho)
        return _shape_like(hist.combine(z, zero, b, 1.0), vec)
    finally:
        hist.d = d


def _dtype_code(dtype):
    if dtype == torch.float32:
        return _lib.RIME_F32
    if dtype == torch.float64:
        return _lib.RIME_F64
    raise TypeError('bfgs: float32 / float64 (or complex64 / complex128) vectors only, got %s' % dtype)


def _real_view(t):
    """the contiguous 1-D real vector the kernels read: t itself, or the interleaved view of a complex t"""
    if t.ndim != 1:
        t = t.reshape(-1)
    if not t.is_contiguous():
        t = t.contiguous()
    if t.is_conj():
        t = t.resolve_conj()
    return torch.view_as_real(t).reshape(-1) if t.is_complex() else t


def _split_H0(H0, numel, dtype, device):
    """(gamma, d) of a starting matrix gamma * diag(d) for `numel` parameters of `dtype` on `device`: None -> (1, None), a 0-d
    tensor -> (its value, None), a 1-d tensor -> (1, the diagonal as a real vector, repeated per component for a complex dtype)"""
    if H0 is None:
        return 1.0, None
    if _is_operator(H0):
        return 1.0, None
    if isinstance(H0, torch.Tensor) and not H0.is_complex():
        if H0.ndim == 0 or (H0.ndim == 1 and H0.numel() == 1 and numel != 1):
            return float(H0), None
        if H0.ndim == 1:
            if H0.numel() != numel:
                raise ValueError('bfgs: a diagonal H0 of %d elements for %d parameters' % (H0.numel(), numel))
            d = H0.detach().to(device=device, dtype=torch.empty(0, dtype=dtype).real.dtype)
            if dtype.is_complex:
                d = d.repeat_interleave(2)
            return 1.0, d.contiguous()
    raise NotImplementedError('bfgs: H0 must be None, a real 0-d tensor (scalar), a real 1-d tensor (diagonal) or an hmat '
                              'operator (hmat.DiagMat, SparseMat, PartitionedMat, HierMat, ...)')


class _History:
    """the pairs as the kernels see them: real views, the two device tables of their addresses, and the launches"""

    def __init__(self, N, dtype, device, d):
        if torch.device(device).type != 'cuda':
            raise RuntimeError("bayeslim_amd ops need tensors on the GPU (got device '%s'); there is no CPU implementation" % device)
        self.N, self.dtype, self.device, self.d = N, dtype, device, d
        self.code = _dtype_code(dtype)
        self.s, self.y = [], []                    # real views, oldest first (they keep the storage alive)
        self.table = None
        self.ws = None

    def check(self, t):
        _require_cuda(t)
        if t.dtype != self.dtype or t.numel() != self.N or t.device != self.device:
            raise ValueError('bfgs: a vector of %s [%d] on %s where %s [%d] on %s is needed'
                             % (t.dtype, t.numel(), t.device, self.dtype, self.N, self.device))
        return t

    def set_rows(self, s, y):
        self.s, self.y = [self.check(_real_view(t)) for t in s], [self.check(_real_view(t)) for t in y]
        m = len(self.s)
        if m:
            ptrs = [t.data_ptr() for t in self.s] + [t.data_ptr() for t in self.y]
            self.table = torch.tensor(ptrs, dtype=torch.int64).to(self.device)
            nbytes = int(_lib.lib.rime_lbfgs_workspace(m, self.N))
            if self.ws is None or self.ws.numel() * 8 < nbytes:
                self.ws = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)

    def _tables(self):
        m = len(self.s)
        return ctypes.c_void_p(self.table.data_ptr()), ctypes.c_void_p(self.table.data_ptr() + 8 * m), m

    def dots(self, v, k=-1):
        """(2 or 5, m) float64 numpy array of rime_lbfgs_dots for the vector v (a real view)"""
        S, Y, m = self._tables()
        out = torch.empty((5 if k >= 0 else 2, m), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.rime_lbfgs_dots(self.code, S, Y, m, self.N, _ptr(self.check(v)), _ptr(self.d), k, _ptr(out),
                                                _ptr(self.ws), self.ws.numel() * 8, _stream()), 'rime_lbfgs_dots')
        return out.cpu().numpy()

    def combine(self, v, a, b, gamma):
        S, Y, m = self._tables()
        ab = torch.as_tensor(np.stack([a, b])).to(self.device)
        r = torch.empty_like(v)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.rime_lbfgs_combine(self.code, S, Y, m, self.N, _ptr(self.check(v)), _ptr(self.d), _ptr(ab[0]),
                                                   _ptr(ab[1]), float(gamma), _ptr(r), _stream()), 'rime_lbfgs_combine')
        return r


def _shape_like(r, vec):
    return torch.view_as_complex(r.reshape(-1, 2)) if vec.is_complex() else r


def _start(vec, d, gamma):
    """gamma * d o vec without a history (nothing to fuse: one elementwise product)"""
    r = _real_view(vec)
    return _shape_like(r * gamma if d is None else (gamma * d) * r, vec)


def two_loop_recursion(vec, s, y, rho, H0=None):
    """
    The product of the implicit L-BFGS matrix defined by s, y, rho and H0 with vec (reference bfgs.two_loop_recursion), on
    the kernels.  s, y: sequences of tensors, oldest first; rho: sequence of 1 / (s_i . y_i); H0: None, a 0-d tensor or a
    1-d tensor (the diagonal), or an hmat operator.  The Gram matrices are formed here from len(s) dots launches; LBFGS.hvp keeps
    them instead.
    """
    _require_cuda(vec)
    gamma, d = _split_H0(H0, vec.numel(), vec.dtype, vec.device)
    m = len(s)
    if m == 0:
        return H0(vec) if _is_operator(H0) else _start(vec, d, gamma)
    v = _real_view(vec)
    hist = _History(v.numel(), v.dtype, v.device, d)
    hist.set_rows(list(s), list(y))
    SY, YDY = np.zeros((m, m)), np.zeros((m, m))
    for k in range(m):
        out = hist.dots(v, k)
        SY[:, k], YDY[:, k] = out[2], out[4]
    if _is_operator(H0):
        return _operator_direction(hist, H0, 1.0, vec, SY, out[0], rho=rho)
    a, b = compact_coeffs(SY, YDY, out[0], out[1], gamma, rho=rho)
    return _shape_like(hist.combine(v, a, b, gamma), vec)


class _QuasiNewton:
    """what LBFGS and BFGS share: the flat view of the parameters and the iteration of step().  A subclass gives the search
    direction for a gradient (_step_direction) and takes the new pair together with the gradient of the next direction
    (_step_update)."""

    # ------------------------------------------------------------------ parameters
    def _numel(self):
        if self._numel_cache is None:
            self._numel_cache = sum(p.numel() for p in self.params)
        return self._numel_cache

    def gather_flat_grad(self):
        views = []
        for p in self.params:
            if p.grad is None:
                views.append(p.new_zeros(p.numel()))
            elif p.grad.is_sparse:
                views.append(p.grad.to_dense().reshape(-1))
            else:
                views.append(p.grad.reshape(-1))
        return torch.cat(views, dim=0)

    def update_params(self, step_size, update):
        """move the parameters along the flat direction `update` by `step_size`"""
        offset = 0
        for p in self.params:
            n = p.numel()
            p.add_(update[offset:offset + n].view_as(p), alpha=step_size)
            offset += n
        assert offset == self._numel()

    def clone_param(self):
        return [p.clone(memory_format=torch.contiguous_format) for p in self.params]

    def set_param(self, params_data):
        for p, pdata in zip(self.params, params_data):
            p.copy_(pdata)

    def directional_evaluate(self, closure, x, alpha, p):
        """loss and flat gradient at x + alpha p; the parameters are x again afterwards"""
        self.update_params(alpha, p)
        loss = float(closure())
        flat_grad = self.gather_flat_grad()
        self.set_param(x)
        return loss, flat_grad

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    if p.grad.grad_fn is not None:
                        p.grad.detach_()
                    else:
                        p.grad.requires_grad_(False)
                    p.grad.zero_()

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure):
        """up to max_iter iterations; closure evaluates the model, fills the gradients and returns the loss"""
        self._exit = 0
        closure = torch.enable_grad()(closure)
        current_evals = 0
        if self._loss is None:
            loss = float(closure())
            current_evals += 1
            flat_grad = self.gather_flat_grad()
        else:
            loss, flat_grad = self._loss, self._flat_grad
        is_finite = math.isfinite(loss) and bool(torch.isfinite(flat_grad.sum()))
        if bool(flat_grad.abs().max() <= self.tolerance_grad) or not is_finite:
            self._exit = 2
            return loss

        n_iter = 0
        while n_iter < self.max_iter:
            p = self._step_direction(flat_grad)

            if self.n_iter == 0 and self.line_search_fn is None:
                alpha = float(min(1., 1. / flat_grad.abs().sum())) * self.lr
            else:
                alpha = self.lr

            gp = float((flat_grad.conj() @ p).real)
            if gp > -self.tolerance_change:
                self._exit = 1
                break

            prev_loss, prev_grad = loss, flat_grad
            if self.line_search_fn is None:
                self.update_params(alpha, p)
                loss = float(closure())
                flat_grad = self.gather_flat_grad()
                ls_func_evals = 1
            elif self.line_search_fn == 'strong_wolfe':
                x = self.clone_param()

                def obj_func(x, alpha, p):
                    return self.directional_evaluate(closure, x, alpha, p)

                loss, flat_grad, alpha, ls_func_evals = strong_wolfe(
                    obj_func, x, alpha, p, loss, flat_grad, gp, tolerance_change=self.tolerance_change, max_ls=self.max_ls_eval)
                alpha = float(alpha)
                self.update_params(alpha, p)
            else:
                raise NameError("didn't recognize line_search {}".format(self.line_search_fn))
            opt_cond = bool(flat_grad.abs().max() <= self.tolerance_grad)
            current_evals += ls_func_evals
            self.func_evals += ls_func_evals

            if opt_cond:
                self._exit = 2
                break
            if float(p.mul(alpha).abs().max()) <= self.tolerance_change:
                self._exit = 3
                break
            if abs(loss - prev_loss) < self.tolerance_change:
                self._exit = 4
                break

            s = alpha * p
            y = flat_grad - prev_grad
            self._step_update(s, y, alpha, flat_grad, p)

            n_iter += 1
            self.n_iter += 1

        self._loss = loss
        self._flat_grad = flat_grad
        return loss



class LBFGS(_QuasiNewton):
    """
    Limited-memory BFGS (Nocedal & Wright, Numerical Optimization, 2nd ed., algorithm 7.4 and 7.5) with the interface of the
    reference's bfgs.LBFGS.  All parameters live on one GPU.

    H0: None (identity), a 0-d tensor (scalar), a 1-d tensor (diagonal) or an hmat operator -- the starting inverse Hessian,
    kept as gamma * diag(d), or as gamma * H0 with d the operator's diagonal: with update_Hdiag the scalar gamma is reset to (y . s) / (y . d o y) whenever a pair is stored (eqn 7.20
    with the given diagonal as the metric), which is the reference's scalar_mul applied to H and _Hdiag together.
    _exit after step(): 0 max_iter reached, 1 directional derivative above -tolerance_change, 2 gradient below tolerance_grad
    (or not finite), 3 step below tolerance_change, 4 loss change below tolerance_change.
    """
    _history_cls = _History            # what holds the pairs and runs the two passes (the tests put a float64 oracle here)

    def __init__(self, params, H0=None, lr=1.0, max_iter=10, max_ls_eval=10, history_size=100, tolerance_grad=1e-14,
                 tolerance_change=1e-16, line_search_fn='strong_wolfe', store_Hy=False, update_Hdiag=True):
        self.update_Hdiag = update_Hdiag
        self.history_size = history_size
        self.lr = lr
        self.max_iter = max_iter
        self.max_ls_eval = max_ls_eval
        self.tolerance_grad = tolerance_grad
        self.tolerance_change = tolerance_change
        self.line_search_fn = line_search_fn
        self.store_Hy = store_Hy
        self.params = list(params)
        self.func_evals = 0
        self.n_iter = 0
        self._loss = None
        self._flat_grad = None
        self._numel_cache = None
        self._exit = None
        self._g = None
        self._s, self._y, self._Hy = deque(), deque(), deque()
        self._rho, self._alpha = [], []
        self._init_H(H0)

    # ------------------------------------------------------------------ starting matrix and history
    def _init_H(self, H0):
        p0 = self.params[0]
        gamma, d = _split_H0(H0, self._numel(), p0.dtype, p0.device)
        self.H = H0
        self._op = H0 if _is_operator(H0) else None
        self._complex = p0.is_complex()
        rdt = p0.real.dtype if self._complex else p0.dtype
        if self._op is not None and self.update_Hdiag:
            # the metric of eqn 7.20: the operator's diagonal, as the reference's _Hdiag
            d = self._op.diagonal().real.detach().to(device=p0.device, dtype=rdt)
            d = (d.repeat_interleave(2) if self._complex else d).contiguous()
        self._gamma, self._d = gamma, d
        self._hist = self._history_cls(self._numel() * (2 if self._complex else 1), rdt, p0.device, d)
        self._SY, self._YDY = np.zeros((0, 0)), np.zeros((0, 0))
        self._pending = None

    @property
    def _Hdiag(self):
        """the diagonal of the current starting matrix (ones without update_Hdiag, as in the reference)"""
        n, dev = self._numel(), self.params[0].device
        if not self.update_Hdiag:
            return torch.ones(n, dtype=self._hist.dtype, device=dev)
        d = self._d if self._d is None or not self._complex else self._d[::2]
        return torch.full((n,), self._gamma, dtype=self._hist.dtype, device=dev) if d is None else self._gamma * d

    def _set_history(self, s, y, idx):
        """keep the pairs `idx` of the candidate lists s, y (and of the Gram matrices, which cover the candidates)"""
        self._s, self._y = deque(s[i] for i in idx), deque(y[i] for i in idx)
        self._SY, self._YDY = self._SY[np.ix_(idx, idx)], self._YDY[np.ix_(idx, idx)]
        self._hist.set_rows(list(self._s), list(self._y))

    def _update(self, s, y, alpha, v):
        """
        Offer the pair (s, y); v (a real view) is the vector whose inner products with the history come from the same
        launch.  Returns (Sv, YDv) over the pairs kept -- with or without the new one.
        """
        Hy = self.hvp(y) if self.store_Hy else None
        s_all, y_all = list(self._s) + [s], list(self._y) + [y]
        m = len(s_all)
        k = m - 1
        self._hist.set_rows(s_all, y_all)
        out = self._hist.dots(v, k)
        ys = out[2, k]
        self._pending = None
        if not ys > self.tolerance_grad:
            # not enough curvature: the pair is not stored; history, Gram matrices and gamma stay as they were
            self._hist.set_rows(list(self._s), list(self._y))
            return out[0, :k], out[1, :k]
        SY, YDY = np.zeros((m, m)), np.zeros((m, m))
        SY[:k, :k], YDY[:k, :k] = self._SY, self._YDY
        SY[:, k], SY[k, :] = out[2], out[3]
        YDY[:, k], YDY[k, :] = out[4], out[4]
        self._SY, self._YDY = SY, YDY
        keep = list(range(1, m)) if m > self.history_size else list(range(m))
        if len(keep) < m:
            self._rho, self._alpha = self._rho[1:], self._alpha[1:]
            if self.store_Hy:
                self._Hy.popleft()
        self._set_history(s_all, y_all, keep)
        self._rho.append(1.0 / ys)
        self._alpha.append(alpha)
        self._g = self.gather_flat_grad()
        if self.store_Hy:
            self._Hy.append(Hy)
        if self.update_Hdiag:
            self._gamma = float(ys / out[4, k])
        return out[0, keep], out[1, keep]

    def update_hessian(self, s, y, alpha=None):
        """store the pair (s, y) if it has enough curvature, 1 / rho = y . s > tolerance_grad (reference LBFGS.update_hessian)"""
        self._update(s, y, alpha, _real_view(y))

    def _direction(self, vec, dots=None):
        if self._op is not None and len(self._s) == 0:
            return hmat._apply(self._op, vec, scalar=None if self._gamma == 1.0 else self._gamma)
        if len(self._s) == 0:
            return _start(vec, self._d, self._gamma)
        v = _real_view(vec)
        Sv, YDv = self._hist.dots(v) if dots is None else dots
        if self._op is not None:
            return _operator_direction(self._hist, self._op, self._gamma, vec, self._SY, Sv)
        a, b = compact_coeffs(self._SY, self._YDY, Sv, YDv, self._gamma)
        return _shape_like(self._hist.combine(v, a, b, self._gamma), vec)

    def hvp(self, vec):
        """implicit inverse-Hessian vector product (reference LBFGS.hvp)"""
        return self._direction(vec)

    # ------------------------------------------------------------------ the hooks of step()
    def _step_direction(self, flat_grad):
        # the inner products of this gradient with the history came with the last update, when there was one
        dots = self._pending[1] if self._pending is not None and self._pending[0] is flat_grad else None
        return -self._direction(flat_grad, dots)

    def _step_update(self, s, y, alpha, flat_grad, p):
        # new pair and the inner products of the next direction from ONE dots launch
        self._pending = (flat_grad, self._update(s, y, alpha, _real_view(flat_grad)))


# ============================================================================================================== dense BFGS
class _Dense:
    """the two passes of csrc/bfgs.hip over a real matrix H [N][ld] (a 2-d tensor with unit column stride)"""

    def __init__(self, N, dtype, device):
        if torch.device(device).type != 'cuda':
            raise RuntimeError("bayeslim_amd ops need tensors on the GPU (got device '%s'); there is no CPU implementation" % device)
        self.N, self.dtype, self.device = N, dtype, torch.device(device)
        self.code = _dtype_code(dtype)

    def _matrix(self, H):
        _require_cuda(H)
        if H.ndim != 2 or H.shape != (self.N, self.N) or H.dtype != self.dtype or H.device != self.device:
            raise ValueError('bfgs: a matrix of %s %s on %s where %s (%d, %d) on %s is needed'
                             % (H.dtype, tuple(H.shape), H.device, self.dtype, self.N, self.N, self.device))
        if self.N > 1 and (H.stride(1) != 1 or H.stride(0) < self.N):
            raise ValueError('bfgs: the rows of the matrix must be contiguous (strides %s)' % (H.stride(),))
        return H, (H.stride(0) if self.N > 1 else 1)

    def _vector(self, x):
        _require_cuda(x)
        if x.dtype != self.dtype or x.shape[0] != self.N or x.device != self.device:
            raise ValueError('bfgs: a vector of %s %s on %s where %s [%d] on %s is needed'
                             % (x.dtype, tuple(x.shape), x.device, self.dtype, self.N, self.device))
        return x.contiguous()

    def matvec(self, H, x):
        """H x for x (N,) or, the interleaved view of a complex vector, (N, 2)"""
        H, ld = self._matrix(H)
        x = self._vector(x)
        r = torch.empty_like(x)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.rime_bfgs_matvec(self.code, _ptr(H), ld, self.N, _ptr(x), x.numel() // self.N, _ptr(r), _stream()),
                       'rime_bfgs_matvec')
        return r

    def rank2(self, H, x, z, a, b):
        """H += a (x z^T + z x^T) + b x x^T, in place"""
        H, ld = self._matrix(H)
        x, z = self._vector(x.reshape(-1)), self._vector(z.reshape(-1))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.rime_bfgs_rank2(self.code, _ptr(H), ld, self.N, _ptr(x), _ptr(z), float(a), float(b), _stream()),
                       'rime_bfgs_rank2')
        return H


class BFGS(_QuasiNewton):
    """
    BFGS with the dense inverse Hessian self.H (Nocedal & Wright, algorithm 6.1), the interface of the reference's bfgs.BFGS.
    All parameters are real (float32 or float64) and live on one GPU.

    H0: None (identity), a scalar or 0-d tensor, or a real SYMMETRIC (N, N) tensor: the update applies H y for y^T H as well,
    so an H0 with max|H0 - H0^T| > 1e-6 max|H0| is refused.  self.H is a private (N, N) copy in the parameters' dtype, updated
    in place (module docstring); the caller's H0 is never written.  _exit after step() as for LBFGS.
    step() launches one product and one correction per completed iteration, and one more product for the first direction
    after the optimiser is made or update_hessian is called from outside; store_Hy adds the product H_{k+1} y_k per
    iteration, cached as _Hy with _s, _y, _rho, _alpha, _g of the last accepted pair (as the reference caches them).
    """
    _dense_cls = _Dense                # what runs the two passes over H (the tests put a float64 oracle here)

    def __init__(self, params, H0=None, lr=1.0, max_iter=20, max_ls_eval=10, tolerance_grad=1e-14, tolerance_change=1e-16,
                 line_search_fn='strong_wolfe', store_Hy=False):
        self.lr = lr
        self.max_iter = max_iter
        self.max_ls_eval = max_ls_eval
        self.tolerance_grad = tolerance_grad
        self.tolerance_change = tolerance_change
        self.line_search_fn = line_search_fn
        self.store_Hy = store_Hy
        self.params = list(params)
        self.func_evals = 0
        self.n_iter = 0
        self._loss = None
        self._flat_grad = None
        self._numel_cache = None
        self._exit = None
        self._alpha = self._rho = None
        self._s = self._y = self._g = self._Hy = None
        self._init_H(H0)

    def _init_H(self, H0):
        p0, N = self.params[0], self._numel()
        if any(p.is_complex() for p in self.params):
            raise NotImplementedError('bfgs.BFGS: complex parameters are not supported (optimise their real view)')
        self._dense = self._dense_cls(N, p0.dtype, p0.device)
        if H0 is None:
            H0 = 1.0
        if isinstance(H0, torch.Tensor) and H0.ndim == 2:
            if H0.is_complex() or tuple(H0.shape) != (N, N):
                raise ValueError('bfgs.BFGS: H0 must be a real (%d, %d) tensor, got %s %s' % (N, N, H0.dtype, tuple(H0.shape)))
            H0 = H0.detach()
            if float((H0 - H0.T).abs().max()) > 1e-6 * float(H0.abs().max()):
                raise ValueError('bfgs.BFGS: H0 must be symmetric (max|H0 - H0^T| > 1e-6 max|H0|)')
            self.H = H0.to(device=p0.device, dtype=p0.dtype).clone(memory_format=torch.contiguous_format)
        elif isinstance(H0, (int, float)) or (isinstance(H0, torch.Tensor) and H0.numel() == 1 and not H0.is_complex()):
            self.H = torch.zeros(N, N, dtype=p0.dtype, device=p0.device)
            self.H.diagonal().fill_(float(H0))
        else:
            raise ValueError('bfgs.BFGS: H0 must be None, a real scalar or 0-d tensor, or a real (N, N) tensor')
        self._Hg = None                    # (gradient, H gradient) of the next direction, when step() has it

    def hvp(self, vec):
        """inverse-Hessian vector product H vec; a complex vec as (H Re vec) + i (H Im vec) in one pass (reference BFGS.hvp)"""
        if vec.is_complex():
            r = self._dense.matvec(self.H, torch.view_as_real(vec.resolve_conj().contiguous()))
            return torch.view_as_complex(r)
        return self._dense.matvec(self.H, vec)

    def update_hessian(self, s, y, alpha=None, Hy=None):
        """
        The BFGS update of self.H by the pair (s, y) if it has enough curvature, 1 / rho = y . s > tolerance_grad (reference
        BFGS.update_hessian); alpha is only cached.  Hy: the product H y where the caller has it already (step() does).
        Returns None for a refused pair and (rho, b) of the correction H += -rho (s w^T + w s^T) + b s s^T, w = H y, otherwise.
        """
        if Hy is None:
            ys = float(y @ s)
            if not ys > self.tolerance_grad:
                return None
            Hy = self.hvp(y)
            theta = float(y @ Hy)
        else:
            ys, theta = torch.stack([y @ s, y @ Hy]).tolist()
            if not ys > self.tolerance_grad:
                return None
        rho = 1.0 / ys
        b = rho * rho * theta + rho
        self._dense.rank2(self.H, s, Hy, -rho, b)
        self._Hg = None
        self._s, self._y, self._rho, self._alpha = s, y, rho, alpha
        if self.store_Hy:
            self._Hy = self.hvp(y)
        self._g = self.gather_flat_grad()
        return rho, b

    # ------------------------------------------------------------------ the hooks of step()
    def _step_direction(self, flat_grad):
        if self._Hg is None or self._Hg[0] is not flat_grad:
            self._Hg = (flat_grad, self.hvp(flat_grad))
        return -self._Hg[1]

    def _step_update(self, s, y, alpha, flat_grad, p):
        # p = -H_k g_k, so H_k y = H_k g_{k+1} + p; H_{k+1} g_{k+1} from u, w, s (module docstring)
        u = self.hvp(flat_grad)
        w = u + p
        applied = self.update_hessian(s, y, alpha, Hy=w)
        if applied is not None:
            rho, b = applied
            sg, wg = torch.stack([s @ flat_grad, w @ flat_grad]).tolist()
            u = u.add(s, alpha=b * sg - rho * wg).add_(w, alpha=-rho * sg)
        self._Hg = (flat_grad, u)


def _dense_start(H0, N, dtype, device):
    """a dense (N, N) copy of a starting matrix: None, a scalar, a diagonal, a matrix or an hmat operator"""
    if _is_operator(H0):
        H0 = H0.to_dense()
    if H0 is None:
        return torch.eye(N, dtype=dtype, device=device)
    H0 = torch.as_tensor(H0).detach().to(device=device, dtype=dtype)
    if H0.ndim < 2:
        H0 = torch.atleast_1d(H0)
        return torch.diag(H0) if len(H0) == N else torch.eye(N, dtype=dtype, device=device) * H0
    return H0.clone()


def implicit_to_dense(H0, s, y):
    """
    The dense inverse Hessian that the BFGS updates by the pairs (s_k, y_k), oldest first, make of H0 (reference
    bfgs.implicit_to_dense): H0 None, a scalar, a 1-d tensor (diagonal), a symmetric (N, N) tensor or an hmat operator.
    """
    N = len(s[0])
    B = BFGS((s[0],), H0=_dense_start(H0, N, s[0].dtype, s[0].device))
    for s_k, y_k in zip(s, y):
        B.update_hessian(s_k, y_k)
    return B.H


# ============================================================================================================ factored form
def factor_pairs(s_k, y_k, g_k, alpha_k, Hy_k, pos=True, rank2=True):
    """
    The pair (u, v) of the product form H_{k+1} = (I + u v^T) H_k (I + u v^T)^T of a quasi-Newton update (Brodlie, Gourlay &
    Greenstadt 1973; reference bfgs.factor_pairs), real vectors, plain torch on the inputs' device.

    s_k, y_k: the pair; g_k: the gradient at x_k; alpha_k: the step length, so that H_k^-1 s_k = -alpha_k g_k; Hy_k = H_k y_k
    (None is allowed for rank2: only the check y . H y >= 0 is lost); pos: the sign of the root; rank2: the BFGS update,
    otherwise the symmetric rank-one update.  Returns (u, v, spd), spd a 0-d bool tensor: the update keeps H positive definite.
    """
    sy = s_k @ y_k
    Bs = -alpha_k * g_k
    sBs = s_k @ Bs
    yHy = None if Hy_k is None else y_k @ Hy_k
    sign = 1.0 if pos else -1.0
    if rank2:
        spd = sy > 0
        if yHy is not None:
            spd = spd & ((sy - yHy) <= sy)
        u = s_k / sy
        v = sign * torch.sqrt(sy / sBs) * Bs - y_k
    else:
        if yHy is None:
            raise ValueError('bfgs.factor_pairs: the rank-one form needs Hy_k')
        ratio = (sBs - sy) / (sy - yHy)
        spd = ratio >= 0
        u = (sign * torch.sqrt(ratio) - 1.0) / (sBs - 2 * sy + yHy) * (s_k - Hy_k)
        v = Bs - y_k
    return u, v, spd


def forward_shell(G, d):
    """c of the chain vec <- vec + u_k (v_k . vec), k = 0 ... m - 1: c_k = d_k + sum_{j < k} G[k, j] c_j with G[k, j] = v_k . u_j and
    d_k = v_k . vec0; the chain gives vec0 + sum_k c_k u_k.  float64 on the host."""
    G, d = np.asarray(G, dtype=np.float64), np.asarray(d, dtype=np.float64)
    c = np.zeros(len(d))
    for k in range(len(d)):
        c[k] = d[k] + G[k, :k] @ c[:k]
    return c


def reverse_shell(G, d):
    """e of the reversed chain vec <- vec + v_k (u_k . vec), k = m - 1 ... 0: e_k = d_k + sum_{j > k} G[j, k] e_j with d_k = u_k . vec0;
    the chain gives vec0 + sum_k e_k v_k.  float64 on the host."""
    G, d = np.asarray(G, dtype=np.float64), np.asarray(d, dtype=np.float64)
    m = len(d)
    e = np.zeros(m)
    for k in range(m - 1, -1, -1):
        e[k] = d[k] + G[k + 1:, k] @ e[k + 1:]
    return e


def _shell_history(u, v):
    """(the tables S = u, Y = v, the Gram matrix G[k, j] = v_k . u_j from the k-indexed outputs of m dots launches)"""
    m = len(u)
    hist = _History(u[0].numel(), u[0].dtype, u[0].device, None)
    hist.set_rows(list(u), list(v))
    G = np.zeros((m, m))
    for k in range(m):
        G[k] = hist.dots(hist.s[0], k)[2]                     # out[2][j] = s_j . y_k = u_j . v_k
    return hist, G


def _apply_start(M, vec):
    """M vec for a real vector: M None, a 1-d tensor (diagonal), a 2-d tensor (rime_bfgs_matvec) or an hmat operator"""
    if M is None:
        return vec
    if _is_operator(M):
        return hmat._apply(M, vec)
    if M.ndim < 2:
        return M * vec
    M = M if M.stride(1) == 1 and M.stride(0) >= M.shape[1] else M.contiguous()
    return _Dense(vec.numel(), vec.dtype, vec.device).matvec(M.to(vec.dtype), vec)


def _shells(vec, M, hist, G, both):
    """(left chain) M (right chain, with `both`) applied to one real vector"""
    _require_cuda(vec)
    if vec.is_complex():
        raise NotImplementedError('bfgs: the factored form serves real vectors only')
    vec = _real_view(vec)
    m = 0 if hist is None else len(hist.s)
    zero = np.zeros(m)
    if both and m:
        vec = hist.combine(vec, -reverse_shell(G, hist.dots(vec)[0]), zero, 1.0)
    vec = _apply_start(M, vec)
    if m:
        vec = hist.combine(vec, zero, forward_shell(G, hist.dots(vec)[1]), 1.0)
    return vec


def _columns(vec, f):
    return f(vec) if vec.ndim == 1 else torch.stack([f(vec[:, i]) for i in range(vec.shape[1])], dim=1)


def factored_lvp(vec, L0, u, v):
    """L vec for L = (I + u_m v_m^T) ... (I + u_1 v_1^T) L0 (reference bfgs.factored_lvp): u, v lists of real vectors, L0 None,
    a 1-d tensor, a 2-d tensor or an hmat operator; a 2-d vec is served column by column"""
    hist, G = _shell_history(u, v) if len(u) else (None, None)
    return _columns(vec, lambda x: _shells(x, L0, hist, G, False))


def factored_hvp(vec, H0, u, v):
    """H vec for H = (I + u_m v_m^T) ... (I + u_1 v_1^T) H0 (I + v_1 u_1^T) ... (I + v_m u_m^T) (reference bfgs.factored_hvp)"""
    hist, G = _shell_history(u, v) if len(u) else (None, None)
    return _columns(vec, lambda x: _shells(x, H0, hist, G, True))


class FactoredInvHessian:
    """
    The factored inverse Hessian H = L L^T of a quasi-Newton run (reference bfgs.FactoredInvHessian): s, y, alpha the lists of
    accepted pairs and step lengths, oldest first, g_end the gradient after the last step (the earlier gradients follow from y),
    Hy the list of H_k y_k (optional for rank2), H0 and its factor L0 (given together) None, 1-d, 2-d or hmat operators.
    Pairs whose update is not positive definite are dropped.  Real vectors only.  The Gram matrix v_k . u_j and the row tables
    of the kept pairs are built once.
    """

    def __init__(self, s, y, g_end, alpha, Hy=None, H0=None, L0=None, rank2=True):
        if H0 is not None and L0 is None:
            raise ValueError("If H0 is fed, L0 should be too")
        if not len(s) == len(y) == len(alpha):
            raise ValueError('bfgs.FactoredInvHessian: s, y and alpha must have one entry per pair')
        self.H0, self.L0, self.rank2 = H0, L0, rank2
        self.m, self.N, self.device = len(s), len(s[0]), s[0].device
        g = [None] * self.m
        for i in range(self.m - 1, -1, -1):                   # g_k = g_{k+1} - y_k
            g_end = g_end - y[i]
            g[i] = g_end
        Hy = [None] * self.m if Hy is None else Hy
        self.u, self.v = [], []
        for k in range(self.m):
            u_k, v_k, spd = factor_pairs(s[k], y[k], g[k], alpha[k], Hy[k], pos=True, rank2=rank2)
            if bool(spd):
                self.u.append(u_k)
                self.v.append(v_k)
        self._hist = self._G = None

    def _shell(self):
        if self._hist is None and len(self.u):
            self._hist, self._G = _shell_history(self.u, self.v)
        return self._hist, self._G

    def push(self, device):
        """move the vectors and the starting matrices to a device (or dtype)"""
        from . import utils
        if not isinstance(device, torch.dtype):
            self.device = device
        for M in (self.H0, self.L0):
            if _is_operator(M):
                M.push(device)
        self.H0 = self.H0 if self.H0 is None or _is_operator(self.H0) else utils.push(self.H0, device)
        self.L0 = self.L0 if self.L0 is None or _is_operator(self.L0) else utils.push(self.L0, device)
        self.u, self.v = [utils.push(t, device) for t in self.u], [utils.push(t, device) for t in self.v]
        self._hist = self._G = None

    def hvp(self, vec):
        """inverse-Hessian vector product"""
        hist, G = self._shell()
        return _columns(vec, lambda x: _shells(x, self.H0, hist, G, True))

    def lvp(self, vec):
        """factor vector product: lvp of a standard normal vector is a sample with covariance H"""
        hist, G = self._shell()
        return _columns(vec, lambda x: _shells(x, self.L0, hist, G, False))

    __call__ = lvp

    def to_dense(self, hess=True):
        """the dense H (every shell one product and one rime_bfgs_rank2 pass) or, hess=False, the dense L (torch products)"""
        if not len(self.u):
            return _dense_start(self.H0 if hess else self.L0, self.N, torch.get_default_dtype(), self.device)
        dtype = self.u[0].dtype
        M = _dense_start(self.H0 if hess else self.L0, self.N, dtype, self.device)
        if not hess:
            for u, v in zip(self.u, self.v):
                M = torch.addr(M, u, v @ M)
            return M
        M = M.contiguous()
        dense = _Dense(self.N, dtype, self.device)
        for u, v in zip(self.u, self.v):
            z = dense.matvec(M, v)
            dense.rank2(M, u, z, 1.0, float(v @ z))
        return M


def lbfgs_approx_cov(prob, Nsteps=5, max_iter=1, lr=1e-5, tolerance_grad=1e-40, tolerance_change=1e-40, **kwargs):
    """
    The diagonal L-BFGS estimate of the inverse Hessian (Nocedal & Wright eqn 6.20 through LBFGS._Hdiag) of every parameter
    group of prob.main_params on its own (reference bfgs.lbfgs_approx_cov): prob is an optim.LogProb whose main parameters
    are set; each group in turn becomes the only main parameter and takes Nsteps calls of LBFGS.step(prob.closure) with
    max_iter iterations each; the groups are restored afterwards (the parameter VALUES move with the optimisation).  lr,
    tolerance_grad and tolerance_change are accepted for the reference's signature and, as there, not passed on; kwargs go to
    LBFGS.  Returns hmat.DiagMat of the concatenated diagonals.
    """
    if prob.main_params is None:
        raise ValueError('bfgs.lbfgs_approx_cov: prob.set_main_params(...) first')
    groups = [(prob._main_names[k], idx, k) for k, idx in prob._main_index.items()]
    diags = []
    for group in groups:
        prob.set_main_params()
        prob.unset_param(prob.named_params)
        prob.set_main_params([group])
        opt = LBFGS((prob.main_params,), update_Hdiag=True, max_iter=max_iter, **kwargs)
        for _ in range(Nsteps):
            opt.step(prob.closure)
        diags.append(opt._Hdiag)
    prob.set_main_params()
    prob.unset_param(prob.named_params)
    prob.set_main_params(groups)
    return hmat.DiagMat(torch.cat(diags))


def cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds=None):
    """
    Minimiser of the cubic through (x1, f1) and (x2, f2) with slopes g1, g2, clipped to bounds (default: the interval
    between the points); the midpoint of the bounds when the cubic has no real stationary point.  Floats or 0-d tensors.
    """
    if bounds is not None:
        lo, hi = bounds
    elif x1 <= x2:
        lo, hi = x1, x2
    else:
        lo, hi = x2, x1
    d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2)
    d2_square = d1 ** 2 - g1 * g2
    if not d2_square >= 0:
        return (lo + hi) / 2.
    d2 = d2_square.sqrt() if isinstance(d2_square, torch.Tensor) else math.sqrt(d2_square)
    if x1 <= x2:
        min_pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2))
    else:
        min_pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2))
    return min(max(min_pos, lo), hi)


def strong_wolfe(obj_func, x, alpha, p, f, g, gp, c1=1e-4, c2=0.9, tolerance_change=1e-9, max_ls=25):
    """
    Line search for a step satisfying the strong Wolfe conditions (Nocedal & Wright, algorithms 3.5 and 3.6, in the
    arrangement of torch.optim.lbfgs that the reference uses): a bracketing phase that grows the step by cubic
    extrapolation, then a zoom phase that shrinks the bracket by cubic interpolation, guarded against stalling at an end.

    obj_func(x, alpha, p) -> (loss, flat gradient) at x + alpha p;  x: what obj_func takes as the starting point;  p: flat
    direction;  f, g, gp: loss, flat gradient and directional derivative g . p at x.  Scalars are handled as Python floats
    (one read-back per evaluation).  Returns (f_new, g_new, alpha, evaluations).
    """
    f, gp = float(f), float(gp)
    p_norm = float(p.abs().max())
    g = g.clone(memory_format=torch.contiguous_format)

    def evaluate(a):
        fa, ga = obj_func(x, a, p)
        return float(fa), ga, float(ga.dot(p.conj()).real)

    f_new, g_new, gp_new = evaluate(alpha)
    ls_func_evals = 1

    # bracketing
    alpha_prev, f_prev, g_prev, gp_prev = 0, f, g, gp
    done = False
    ls_iter = 0
    while ls_iter < max_ls:
        if f_new > (f + c1 * alpha * gp) or (ls_iter > 1 and f_new >= f_prev) or (abs(gp_new) > -c2 * gp and gp_new >= 0):
            # sufficient decrease fails, or the slope turned positive: a minimiser lies between the last two trials
            bracket = [alpha_prev, alpha]
            bracket_f = [f_prev, f_new]
            bracket_g = [g_prev, g_new.clone(memory_format=torch.contiguous_format)]
            bracket_gp = [gp_prev, gp_new]
            break
        if abs(gp_new) <= -c2 * gp:
            bracket, bracket_f, bracket_g = [alpha], [f_new], [g_new]
            done = True
            break
        # extrapolate
        min_step = alpha + 0.01 * (alpha - alpha_prev)
        max_step = alpha * 10
        last = alpha
        alpha = cubic_interpolate(alpha_prev, f_prev, gp_prev, alpha, f_new, gp_new, bounds=(min_step, max_step))
        alpha_prev, f_prev, gp_prev = last, f_new, gp_new
        g_prev = g_new.clone(memory_format=torch.contiguous_format)
        f_new, g_new, gp_new = evaluate(alpha)
        ls_func_evals += 1
        ls_iter += 1

    if ls_iter == max_ls:
        bracket, bracket_f, bracket_g = [0, alpha], [f, f_new], [g, g_new]

    # zoom
    stalled = False
    low, high = (0, 1) if bracket_f[0] <= bracket_f[-1] else (1, 0)
    while not done and ls_iter < max_ls:
        if abs(bracket[1] - bracket[0]) * p_norm < tolerance_change:
            break
        alpha = cubic_interpolate(bracket[0], bracket_f[0], bracket_gp[0], bracket[1], bracket_f[1], bracket_gp[1])
        # a trial within a tenth of the bracket from an end: accept it once, then step a tenth in from the nearer end
        top, bottom = max(bracket), min(bracket)
        eps = 0.1 * (top - bottom)
        if min(top - alpha, alpha - bottom) < eps:
            if stalled or alpha >= top or alpha <= bottom:
                alpha = top - eps if abs(alpha - top) < abs(alpha - bottom) else bottom + eps
                stalled = False
            else:
                stalled = True
        else:
            stalled = False

        f_new, g_new, gp_new = evaluate(alpha)
        ls_func_evals += 1
        ls_iter += 1

        if f_new > (f + c1 * alpha * gp) or f_new >= bracket_f[low]:
            bracket[high], bracket_f[high], bracket_gp[high] = alpha, f_new, gp_new
            bracket_g[high] = g_new.clone(memory_format=torch.contiguous_format)
            low, high = (0, 1) if bracket_f[0] <= bracket_f[1] else (1, 0)
        else:
            if abs(gp_new) <= -c2 * gp:
                done = True
            elif gp_new * (bracket[high] - bracket[low]) >= 0:
                bracket[high], bracket_f[high], bracket_gp[high] = bracket[low], bracket_f[low], bracket_gp[low]
                bracket_g[high] = bracket_g[low]
            bracket[low], bracket_f[low], bracket_gp[low] = alpha, f_new, gp_new
            bracket_g[low] = g_new.clone(memory_format=torch.contiguous_format)

    return bracket_f[low], bracket_g[low], bracket[low], ls_func_evals
