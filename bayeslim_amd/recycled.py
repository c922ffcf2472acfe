"""
What sampler.py lists as not provided, for the diagonal-mass sampler: RecycledHMC on the fused kernel of csrc/recycle.hip, the
step-size objects StepSize and DynamicStepSize (complex step sizes), momentum masks (pmask) and estimate_cov: the counterpart of the
reference's sampler.py:516-542, 673-712, 732-919 and 1586-1889.  sampler.HMC, nuts.NUTS and massmat keep refusing all of these in
their own words; the classes that take them live here: recycled.HMC and recycled.RecycledHMC.

RecycledHMC (Nishimura & Dunson 2020) runs Nstep single-step leapfrogs and offers EVERY intermediate state to the Metropolis
test.  Between two gradient evaluations the reference closes step i with a half kick, takes the kinetic energy, clones q and p,
and opens step i + 1 with a half kick and a drift.  Here that is ONE launch of rime_hmc_recycle, which writes the snapshot into
row i of two (Nstep, N) trajectory buffers -- 5 vector reads and 4 writes where rime_hmc_step with the energy, two device copies
and rime_hmc_step take 11 and 5 -- and carries the bits of that sequence (include/rime_hip.h).  A move that does not diverge is
Nstep + 2 launches (the starting energy, the opening stage, Nstep recycle launches), and its accepted rows reach the host chain in
one device-to-host copy.  Extra memory: the two trajectory buffers, 2 * Nstep * N elements of the working precision, allocated
once per sampler.  With a momentum mask the reference multiplies the momentum between the two half kicks, which one fused pass
cannot do: a masked recycled move runs the unfused sequence on rime_hmc_step (RecycledHMC).

A complex step size (StepSize, or a complex tensor per key) scales the real and the imaginary part of a complex parameter
separately (multiply_eps): in the flat real vector of sampler._Layout it is the interleaved (re, im) entries of the step vector,
so the kernels need nothing new.  A complex step or mask of a real parameter is a ValueError.

There is no CPU path.
"""
import copy as _copy
import math

import numpy as np
import torch

from . import _lib, sampler, utils
from .ops import _stream, _ptr
from .paramdict import ParamDict
from .sampler import Potential, _check_vectors, _workspace   # noqa: F401


# ------------------------------------------------------------------------------------------------------------ step sizes
def multiply_eps(x, eps):
    """
    x times a step size or mask (reference sampler.multiply_eps): a complex eps scales the real and the imaginary part of x
    separately, complex(x.real * eps.real, x.imag * eps.imag); anything else is the plain product.
    """
    if isinstance(eps, torch.Tensor) and eps.is_complex():
        if isinstance(x, torch.Tensor) and not x.is_complex():
            raise ValueError('recycled.multiply_eps: a complex step size or mask needs a complex tensor, got %s' % x.dtype)
        return torch.complex(x.real * eps.real, x.imag * eps.imag)
    return x * eps


def _entry(other, k):
    return other[k] if isinstance(other, (ParamDict, dict)) else other


class StepSize(ParamDict):
    """
    A step size per key whose product with a position or momentum ParamDict is multiply_eps, so that a complex step scales the two
    components of a complex parameter separately (reference sampler.StepSize).

    eps * ParamDict -> ParamDict;  eps * (StepSize, dict or number) -> StepSize;  + - / ** act on the nominal values `params`
    key by key; the in-place forms change the held tensors.  other / eps and other - eps return a StepSize of the effective step
    (the reference's two methods fail on a StepSize: they pass a DynamicStepSize's argument to copy()).
    """
    def __init__(self, params):
        super().__init__(params)
        self.is_complex = {k: torch.is_complex(v) for k, v in params.items()}

    def copy(self):
        """a shallow copy: the same tensors in a new object"""
        return StepSize(self.params)

    def _fresh(self):
        """the object a reflected operation on the effective step returns"""
        return self.copy()

    def _with(self, fn, other):
        new = self.copy()
        new.params = {k: fn(self.params[k], _entry(other, k)) for k in self.keys()}
        return new

    def values(self):
        return [self[k] for k in self.params]

    def items(self):
        return list(zip(self.keys(), self.values()))

    def __repr__(self):
        return '%s\n' % type(self).__name__ + '\n'.join("'{}': {}".format(k, str(self[k])) for k in self.params)

    def push(self, device):
        """move (or re-type) every step in place; device may be a dict per key"""
        for k in self.params:
            self.params[k] = utils.push(self.params[k], _entry(device, k))
        self._setup()

    def __mul__(self, other):
        if other.__class__ == ParamDict:                         # a position or momentum: the effective step applies
            return ParamDict({k: multiply_eps(other[k], self[k]) for k in self.keys()})
        return self._with(lambda p, o: multiply_eps(o, p), other)

    def __rmul__(self, other):
        if other.__class__ == ParamDict:                         # ParamDict * eps is the ParamDict's own, plain product
            return ParamDict.__mul__(other, self)
        return self.__mul__(other)

    def __imul__(self, other):
        for k in self.keys():
            p = self.params[k]
            p[:] = multiply_eps(_entry(other, k), p)
        return self

    def __truediv__(self, other):
        return self._with(lambda p, o: p / o, other)

    def __rtruediv__(self, other):
        new = self._fresh()
        new.params = {k: _entry(other, k) / self[k] for k in self.keys()}
        return new

    def __itruediv__(self, other):
        for k in self.keys():
            self.params[k] /= _entry(other, k)
        return self

    __div__, __rdiv__, __idiv__ = __truediv__, __rtruediv__, __itruediv__

    def __add__(self, other):
        return self._with(lambda p, o: p + o, other)

    def __radd__(self, other):
        if other.__class__ == ParamDict:
            return other.__add__(self)
        return self.__add__(other)

    def __iadd__(self, other):
        for k in self.keys():
            self.params[k] += _entry(other, k)
        return self

    def __sub__(self, other):
        return self._with(lambda p, o: p - o, other)

    def __rsub__(self, other):
        new = self._fresh()
        new.params = {k: _entry(other, k) - self[k] for k in self.keys()}
        return new

    def __isub__(self, other):
        for k in self.keys():
            self.params[k] -= _entry(other, k)
        return self

    def __pow__(self, alpha):
        return self._with(lambda p, o: p ** o, alpha)


class DynamicStepSize(StepSize):
    """
    A step size that follows the acceptance probability of the last move (reference sampler.DynamicStepSize): the effective step
    of key k is params[k] * eps_mul[k], on the elements index[k] only if an index is given.  update(prob) multiplies every
    eps_mul by gamma when prob < min_prob, and by alpha, capped at 1, otherwise.  Arithmetic acts on params, not on eps_mul.

    params : dict of nominal steps;  eps_mul : dict of starting multipliers (default 1);  gamma, min_prob, alpha : as above;
    index : dict per key of a slice or an integer tensor;  track : keep every eps_mul seen by update in `chain`;  chain : a list
    to start that record from (copied).
    """
    def __init__(self, params, eps_mul=None, gamma=0.8, min_prob=0.2, alpha=1.25, index=None, track=False, chain=None):
        super().__init__(params)
        if eps_mul is None:
            eps_mul = {k: torch.tensor(1.0, device=v.device) for k, v in params.items()}
        elif not isinstance(eps_mul, (ParamDict, dict)):
            raise TypeError('recycled.DynamicStepSize: eps_mul must be a dict or a ParamDict')
        self.eps_mul = eps_mul
        self.min_prob, self.gamma, self.alpha, self.index, self.track = min_prob, gamma, alpha, index, track
        self.chain = None if not track else ([] if chain is None else list(chain))

    def copy(self, **kwargs):
        """a shallow copy; keyword arguments replace the constructor's"""
        kw = dict(eps_mul=self.eps_mul, gamma=self.gamma, min_prob=self.min_prob, alpha=self.alpha, index=self.index,
                  track=self.track)
        kw.update(kwargs)
        return DynamicStepSize(self.params, **kw)

    def _fresh(self):
        return self.copy(eps_mul=None)                            # the effective step becomes the nominal one

    def __getitem__(self, key):
        if self.index is None:
            return self.params[key] * self.eps_mul[key]
        out = self.params[key].clone()
        out[self.index[key]] *= self.eps_mul[key]
        return out

    def update(self, prob):
        """prob: the acceptance probability [0, 1] of the last move"""
        if self.track:
            self.chain.append(_copy.deepcopy(self.eps_mul))
        for k in list(self.eps_mul.keys()):
            v = self.eps_mul[k]
            self.eps_mul[k] = v * self.gamma if prob < self.min_prob else (v * self.alpha).clip(None, 1.0)

    def push(self, device):
        for k in self.params:
            d = _entry(device, k)
            self.params[k] = utils.push(self.params[k], d)
            self.eps_mul[k] = utils.push(self.eps_mul[k], d)
            if self.index is not None and isinstance(self.index[k], torch.Tensor) and not isinstance(d, torch.dtype):
                self.index[k] = utils.push(self.index[k], d)
        self._setup()


# ------------------------------------------------------------------------------------------------------------ the layout helper
def _per_key(lay, val):
    return {k: (val[k] if isinstance(val, (dict, ParamDict)) else val) for k in lay.keys}


def _is_cplx(v):
    return isinstance(v, torch.Tensor) and v.is_complex()


def _broadcast(lay, v, k, what):
    try:
        return torch.broadcast_to(v.detach().to(lay.device), lay.shapes[k])
    except RuntimeError:
        raise ValueError('recycled: %s[%r] of shape %s does not broadcast to its parameter of shape %s'
                         % (what, k, tuple(v.shape), lay.shapes[k])) from None


def _judge_complex(lay, per_key, what):
    """the keys of `per_key` that hold a complex tensor; each must be a complex parameter"""
    keys = [k for k, v in per_key.items() if _is_cplx(v)]
    for k in keys:
        if not lay.cplx[k]:
            raise ValueError('recycled: a complex %s for the real parameter %r (a complex value scales the real and the imaginary '
                             'part of a complex parameter separately)' % (what, k))
        _broadcast(lay, per_key[k], k, what)
    return keys


def expand_eps(lay, eps, judge_only=False):
    """
    The step size as sampler._Layout.expand returns it -- a float, None or the flat vector -- with a complex step of a complex
    key as the interleaved (re, im) entries of the vector.  Without complex values this IS _Layout.expand, bit for bit; a
    StepSize is read through its __getitem__ (the effective step).  A complex step of a real key is a ValueError.
    """
    per_key = _per_key(lay, eps)
    cplx = _judge_complex(lay, per_key, 'eps')
    if not cplx:
        if judge_only:
            lay.classify(per_key, 'eps')
            return None
        return lay.expand(per_key, 'eps')
    rest = {k: (None if k in cplx else v) for k, v in per_key.items()}
    if judge_only:
        lay.classify(rest, 'eps')
        return None
    flat = lay.expand(rest, 'eps')
    if not isinstance(flat, torch.Tensor):
        flat = torch.full((lay.N,), 1.0 if flat is None else flat, dtype=lay.rdtype, device=lay.device)
    for k in cplx:
        v = _broadcast(lay, per_key[k], k, 'eps').to(torch.complex64 if lay.rdtype == torch.float32 else torch.complex128)
        flat[lay.slices[k]].copy_(torch.view_as_real(v.contiguous()).reshape(-1))
    return flat


def hmc_recycle(q, p, g, eps, c, half, drift, q_out, p_out, energy, ws=None):
    """
    One launch of rime_hmc_recycle on flat real vectors (see include/rime_hip.h): q, p in place; g read; eps, c may be None;
    q_out, p_out the rows that receive the snapshot; energy a float64 tensor of one element; ws the workspace (allocated if None).
    """
    N, code = _check_vectors('recycled', 'hmc_recycle', p, (q, g, eps, c, q_out, p_out), dtype_first=True)
    if q is None or g is None or q_out is None or p_out is None or energy is None:
        raise ValueError('recycled: hmc_recycle needs q, p, g, q_out, p_out and energy')
    ws = _workspace(_lib.lib.rime_hmc_workspace(N), p.device, ws)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib.rime_hmc_recycle(code, N, _ptr(q), _ptr(p), _ptr(g), _ptr(eps), _ptr(c), float(half), float(drift),
                                             _ptr(q_out), _ptr(p_out), _ptr(energy), _ptr(ws), ws.numel() * 8, _stream()),
                   'rime_hmc_recycle')


# ------------------------------------------------------------------------------------------------------------ estimate_cov
def estimate_cov(chain, Nback=None, diag_mass=True, robust=False, eps=None, device=None, dtype=None):
    """
    The Cholesky factor of the sample covariance of a chain (a dict per key of a list of numpy arrays, SamplerBase.chain) over its
    last Nback samples (default: all), per key, as a ParamDict on `device` in `dtype` (default: the CPU and the real precision of
    the samples).

    diag_mass=True : sqrt(var) per element in the parameter's shape (real, also for a complex key: var = mean |x - mean|^2), the
        factor sampler.HMC.set_chol takes;  robust : 1.4826 * median |x - median x| instead (the scaled median absolute
        deviation), real keys only.
    diag_mass=False : cholesky(cov(samples) + eps[k] I), lower, (n, n) over the raveled parameter, real keys only: the factor
        massmat.HMC.set_chol takes;  eps : dict per key of the Tikhonov term (default 0; not a step size).

    The reference's method (sampler.py:673-712) cannot run its robust branch, which names an undefined variable, and wraps its
    results for a parameter of one dimension only; the estimators here are numpy's, in the parameter's shape.
    """
    out = {}
    for k, samples in chain.items():
        x = np.asarray(samples)
        x = x if Nback is None else x[-Nback:]
        if x.shape[0] < 2:
            raise ValueError('recycled.estimate_cov: %r holds %d sample(s); two or more are needed' % (k, x.shape[0]))
        cplx = np.iscomplexobj(x)
        if cplx and (robust or not diag_mass):
            raise ValueError('recycled.estimate_cov: %s takes real parameters only (%r is complex)'
                             % ('robust=True' if diag_mass else 'diag_mass=False', k))
        if diag_mass:
            if robust:
                L = 1.4826 * np.median(np.abs(x - np.median(x, axis=0)), axis=0)
            else:
                L = np.sqrt(np.var(x, axis=0))
            L = torch.as_tensor(L)
        else:
            cov = torch.as_tensor(np.atleast_2d(np.cov(x.reshape(x.shape[0], -1).T)))
            reg = 0 if eps is None else eps[k]
            L = torch.linalg.cholesky(cov + reg * torch.eye(len(cov), dtype=cov.dtype), upper=False)
        out[k] = L.to(device=device, dtype=L.dtype if dtype is None else dtype)
    return ParamDict(out)


# ------------------------------------------------------------------------------------------------------------ the samplers
class HMC(sampler.HMC):
    """
    sampler.HMC (identity or diagonal mass) plus what it refuses:

    eps : also a StepSize or DynamicStepSize, or complex tensors per key (see expand_eps).  With a DynamicStepSize every move
        ends with eps.update(prob), after a divergent move too, and the flat step vector is rebuilt once per move.
    pmask : dict or ParamDict per key of None, a real tensor or a complex tensor (complex keys only) that broadcasts to the
        parameter: the drawn momentum is multiplied by it (multiply_eps) before and after hess_L, in draw_momentum only.
        The reference's HMC also masks inside K(p), in place, at the start and at the end of a move: for a masked move its
        K_end, H_end and acceptance probability are those of the masked final momentum (and, for a mask that is not {0, 1}
        valued, its K_start of the twice-masked draw), where here they are those of the momentum the trajectory ends with.
        RecycledHMC below follows the reference's K().
    estimate_cov : sets the diagonal mass from the chain.
    With a plain real eps and no pmask every bit of a seeded chain is sampler.HMC's.
    """
    def __init__(self, potential_fn, x0, eps, cov_L=None, hess_L=None, diag_mass=True, Nstep=10, pdist=None, pmask=None,
                 dHmax=1000, record_divergences=False, U0=None):
        self._pmask_arg = pmask
        super().__init__(potential_fn, x0, eps, cov_L=cov_L, hess_L=hess_L, diag_mass=diag_mass, Nstep=Nstep, pdist=pdist,
                         pmask=None, dHmax=dHmax, record_divergences=record_divergences, U0=U0)
        self.pmask = self._judge_pmask(self._pmask_arg)
        del self._pmask_arg

    def _judge_mass(self, eps, cov_L, hess_L, diag_mass):
        expand_eps(self._lay, eps, judge_only=True)
        super()._judge_mass(1.0, cov_L, hess_L, diag_mass)
        self._judge_pmask(self._pmask_arg, move=False)

    def _judge_pmask(self, pmask, move=True):
        """the masks per key on the sampler's device (None: no mask at all)"""
        if pmask is None:
            return None
        if not isinstance(pmask, (dict, ParamDict)):
            raise TypeError('recycled.HMC: pmask must be a dict or a ParamDict by key')
        lay = self._lay
        per_key = {k: pmask[k] for k in lay.keys}
        for k, v in per_key.items():
            if v is not None and not isinstance(v, torch.Tensor):
                raise TypeError('recycled.HMC: pmask[%r] must be None or a tensor' % k)
        _judge_complex(lay, per_key, 'pmask')
        for k, v in per_key.items():
            if v is not None:
                _broadcast(lay, v, k, 'pmask')
        if not move:
            return None
        ct = torch.complex64 if lay.rdtype == torch.float32 else torch.complex128
        return {k: (None if v is None else _broadcast(lay, v, k, 'pmask').to(ct if v.is_complex() else lay.rdtype).contiguous())
                for k, v in per_key.items()}

    # ------------------------------------------------------------------ step size
    @property
    def eps(self):
        return self._eps

    @eps.setter
    def eps(self, eps):
        if isinstance(eps, torch.Tensor):
            eps = ParamDict({k: eps for k in self._lay.keys})
        flat = expand_eps(self._lay, eps)
        if flat is None:
            raise ValueError('recycled.HMC: eps is None')
        self._eps, self._eps_flat = eps, flat

    def _update_eps(self, prob):
        """what ends every move with a DynamicStepSize: update it, rebuild the flat step vector"""
        if isinstance(self._eps, DynamicStepSize):
            self._eps.update(prob)
            self._eps_flat = expand_eps(self._lay, self._eps)

    # ------------------------------------------------------------------ momentum masks
    def apply_pmask(self, momentum, pmask=None, inplace=True):
        """multiply a momentum ParamDict by pmask (default: the sampler's), in place or on a deep copy; returns it"""
        pmask = pmask if pmask is not None else self.pmask
        if pmask is not None:
            if not inplace:
                momentum = _copy.deepcopy(momentum)
            for k, p in momentum.items():
                if pmask[k] is not None:
                    p[:] = multiply_eps(p, pmask[k])
        return momentum

    def draw_momentum(self):
        """sampler.HMC.draw_momentum with the mask applied before and after hess_L"""
        if self.pmask is None:
            return super().draw_momentum()
        tr = self._traj
        for k in tr.lay.keys:
            x = self.x[k]
            m = self.pdist[k]() if self.pdist is not None else torch.randn(x.numel(), device=x.device, dtype=x.dtype)
            m = m.reshape(x.shape)
            mask, L = self.pmask[k], self.hess_L[k]
            if mask is not None:
                m = multiply_eps(m, mask)
            if L is not None:
                m = L * m
            if mask is not None:
                m = multiply_eps(m, mask)
            tr.pv[k].copy_(m)
        return tr.pv

    # ------------------------------------------------------------------ the move
    def step(self, sample_p=True):
        accept, prob = super().step(sample_p=sample_p)
        self._update_eps(prob)
        return accept, prob

    def estimate_cov(self, Nback=None, diag_mass=True, robust=False, eps=None):
        """set the diagonal mass from the last Nback samples of the chain: set_chol(cov_L=estimate_cov(chain, ...))"""
        if not diag_mass:
            raise NotImplementedError('recycled.HMC.estimate_cov: diag_mass=False is not provided on the diagonal-mass sampler; '
                                      'recycled.estimate_cov(chain, diag_mass=False) returns the dense factors that '
                                      'massmat.HMC.set_chol takes')
        self.set_chol(cov_L=estimate_cov(self.chain, Nback=Nback, diag_mass=True, robust=robust, eps=eps,
                                         device=self._lay.device, dtype=self._lay.rdtype))


class RecycledHMC(HMC):
    """
    Static-trajectory recycled HMC (reference sampler.RecycledHMC; Nishimura & Dunson 2020): one move runs Nstep single leapfrog
    steps from the current position, then offers every state i of the trajectory to a Metropolis test against the START of the
    move, prob_i = min(1, exp(H_start - H_i)), in order; every accepted state joins the chain, and the last accepted one is the
    next position.  step() appends to the chain and to _acceptances itself; sample() only calls it.  Arguments as recycled.HMC.

    pmask : as the reference's K() does at every step of a recycled trajectory, the mask multiplies the momentum in place after
    the draw and after the closing half kick of every step, before its energy and its snapshot.  One fused pass cannot put a
    product between its two half kicks, so a masked move runs the sequence the kernel fuses: per step rime_hmc_step with the
    closing kick, the product with the flat mask, the energy pass, two device copies and rime_hmc_step with the opening kick and
    the drift (3 Nstep + 1 launches of the kernels of csrc/hmc.hip per move).

    A state whose Hamiltonian exceeds H_start by more than dHmax ends the move: nothing is appended, the sampler restarts from a
    random entry of the chain and step() returns (False, 0).  As in the reference the restart replaces x and _U but keeps the
    gradient last evaluated, which opens the next trajectory.

    Per move: Nstep gradient evaluations (one more when _U or the gradient at x is unknown) and, without a mask, Nstep + 2
    launches; the trajectory is kept in two (Nstep, N) device buffers, 2 * Nstep * N elements, from which the accepted rows go
    to the host in one copy (of the range of rows from the first to the last accepted one).  After step(), `_last` holds K_start, H_start and the list H of the move.
    """
    def __init__(self, potential_fn, x0, eps, cov_L=None, hess_L=None, diag_mass=True, Nstep=10, dHmax=1000,
                 record_divergences=False, pdist=None, pmask=None, U0=None):
        if int(Nstep) < 1:
            raise ValueError('recycled.RecycledHMC: Nstep must be 1 or more')
        super().__init__(potential_fn, x0, eps, cov_L=cov_L, hess_L=hess_L, diag_mass=diag_mass, Nstep=Nstep, pdist=pdist,
                         pmask=pmask, dHmax=dHmax, record_divergences=record_divergences, U0=U0)
        self._rows_q = self._rows_p = None
        # the masks as one flat vector (None: no mask anywhere): a complex mask as interleaved (re, im) entries, like a step
        self._mask_flat = None if self.pmask is None else expand_eps(self._lay, self.pmask)

    def _rows(self):
        """the two trajectory buffers (Nstep, N), allocated once (again only if Nstep was changed); an odd N is padded by one
        element per row, so that every row starts on an even element and a complex key can be viewed in it"""
        lay, n = self._lay, int(self.Nstep)
        if self._rows_q is None or self._rows_q.shape[0] != n:
            self._rows_q = torch.zeros(n, lay.N + (lay.N & 1), dtype=lay.rdtype, device=lay.device)
            self._rows_p = torch.zeros(n, lay.N + (lay.N & 1), dtype=lay.rdtype, device=lay.device)
        return self._rows_q[:, :lay.N], self._rows_p[:, :lay.N]

    def _recycle(self, i, drift):
        """the launch that closes step i into row i and, with drift = 1, opens step i + 1; returns the kinetic energy"""
        tr, eps = self._traj, self._eps_flat
        vec = isinstance(eps, torch.Tensor)
        s = 1.0 if vec else float(eps)
        N = tr.lay.N
        hmc_recycle(tr.q, tr.p, tr.g, eps if vec else None, self._c, 0.5 * s, drift * s, self._rows_q[i, :N], self._rows_p[i, :N],
                    tr.energy, tr.ws)
        tr.launches += 1
        return float(tr.energy)

    def _recycle_masked(self, i, drift):
        """what _recycle fuses, with the mask between the closing kick and the energy and snapshot of step i"""
        tr, N = self._traj, self._traj.lay.N
        tr.stage(self._eps_flat, self._c, 0.5, 0.0)
        tr.p.mul_(self._mask_flat)
        K = tr.kinetic(self._c)
        self._rows_q[i, :N].copy_(tr.q)
        self._rows_p[i, :N].copy_(tr.p)
        if drift:
            tr.stage(self._eps_flat, self._c, 0.5, drift)
        return K

    def _append_rows(self, taken, Us):
        """rows `taken` of the position buffer onto the chain: one device-to-host copy, then what append_chain makes per key"""
        lay = self._lay
        host = self._rows_q[taken[0]:taken[-1] + 1].cpu()        # whole (padded) rows from the first to the last taken: contiguous
        for i in taken:
            for k in lay.keys:
                self.chain[k].append(lay.view(host[i - taken[0], :lay.N], k).clone().numpy())
            self.Uchain.append(Us[i])

    @torch.no_grad()
    def step(self, sample_p=True):
        """one recycled move; returns the last state's (accept, prob) as 0-d tensors"""
        tr, Nstep = self._traj, int(self.Nstep)
        if Nstep < 1:
            raise ValueError('recycled.RecycledHMC: Nstep must be 1 or more')
        rows_q, rows_p = self._rows()
        tr.lay.pack(self.x, tr.q)
        if sample_p:
            self.draw_momentum()
        else:
            tr.lay.pack(self.p, tr.p)
        masked = self._mask_flat is not None
        if masked:
            tr.p.mul_(self._mask_flat)
        K_start = tr.kinetic(self._c) + self._logdetM
        if self._U is None or self._gradU is None:
            with torch.enable_grad():
                self.dUdx(tr.qv)
        U_start, grad_start = self._U, self._gradU
        H_start = K_start + float(U_start)
        tr.set_grad(grad_start)
        tr.stage(self._eps_flat, self._c, 0.5, 1.0)

        Us, grads, Hs = [], [], []
        for i in range(Nstep):
            with torch.enable_grad():
                tr.set_grad(self.dUdx(tr.qv))
            K = (self._recycle_masked if masked else self._recycle)(i, 0.0 if i == Nstep - 1 else 1.0)
            H = float(self._U) + K + self._logdetM
            if self.is_divergent(H_start, H):
                self._last = dict(K_start=K_start, H_start=H_start, H=Hs + [H])
                Nchain = len(self.Uchain)
                if self.record_divergences:
                    self._divergences.append((Nchain, tr.lay.views(rows_q[i]).clone(), tr.lay.views(rows_p[i]).clone()))
                if Nchain > 0:                                   # restart from a random entry of the chain
                    j = np.random.randint(0, Nchain)
                    self._U = self.Uchain[j]
                    self.x = ParamDict({k: torch.as_tensor(self.chain[k][j], device=self.x[k].device) for k in self.x})
                self._update_eps(0.0)
                self._sync_model()
                return torch.tensor(False), torch.tensor(0.0, dtype=torch.float64)
            Us.append(self._U)
            grads.append(self._gradU)
            Hs.append(H)
        self._last = dict(K_start=K_start, H_start=H_start, H=Hs)

        self._U, self._gradU = U_start, grad_start
        taken = []
        for i in range(Nstep):
            d = H_start - Hs[i]
            prob = 1.0 if d >= 0 else math.exp(d) if d == d else float('nan')
            accept = bool(np.random.rand() < prob)
            if accept:
                taken.append(i)
                self._U, self._gradU = Us[i], grads[i]
            self._acceptances.append(accept)
        if taken:
            self._append_rows(taken, Us)
            self.x = tr.lay.views(rows_q[taken[-1]]).clone()
            self.p = tr.lay.views(rows_p[taken[-1]]).clone()
        self._update_eps(prob)
        self._sync_model()
        return torch.tensor(accept), torch.tensor(prob, dtype=torch.float64)

    def _sync_model(self):
        """a Potential's model holds the position the chain holds, not the last state of the trajectory"""
        if isinstance(self.potential_fn, Potential):
            self.potential_fn.prob.update(self.x)

    def sample(self, Nsample, Ncheck=None, outfile=None, description=''):
        """Nsample moves, each appending its accepted states; every Ncheck-th move the chain is written to outfile (npz)"""
        for i in range(Nsample):
            self.step()
            if Ncheck is not None and i > 0 and i % Ncheck == 0:
                assert outfile is not None
                self.write_chain(outfile, overwrite=True, description=description)
        self.accept_ratio = sum(self._acceptances) / len(self._acceptances)
