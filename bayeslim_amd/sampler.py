"""
Posterior sampling by Hamiltonian Monte Carlo on the fused leapfrog kernel of csrc/hmc.hip: the counterpart of the reference's
sampler.py (SamplerBase, HMC, leapfrog, Potential, hoffman_uturn) for an identity or diagonal mass matrix.

One leapfrog stage -- momentum kick, position drift and, on the last stage, the kinetic energy -- is ONE launch of
rime_hmc_step over the flat parameter vector: a trajectory of N steps is N + 1 launches with (kick, drift) = (1/2, 1),
(1, 1) x (N - 1), (1/2, 0), in units of the step size, which is the reference's operation order (half kick, then N - 1 times
drift / gradient / full kick, then drift / gradient / half kick).  Inside a trajectory the position, the momentum and the
gradient live in flat contiguous buffers; the ParamDict entries handed to the potential are views into them, so one launch
serves all keys.  A per-key or per-element step size is one flat vector, rebuilt only when `eps` is assigned; a scalar step
size is folded into the two launch scalars.  Complex parameters pass as their interleaved real views, with a real step size
or Cholesky factor repeated per component.  The kinetic energy is summed in a fixed order (float64 beyond one lane), so a
seeded chain is reproducible bit for bit.  There is no CPU path.

Not provided (each raises NotImplementedError naming what is missing):
  * dense and hmat mass matrices: diag_mass=False, and cov_L / hess_L that are anything but None, a number or a real tensor of
    the parameter's shape (the reference's DenseMat, SolveMat, HierMat, SolveHierMat, DiagMat, ...)
  * pmask (momentum masks)
  * RecycledHMC
  * NUTS with TreeInfo (the natural follow-up: it reuses rime_hmc_step with Nstep = 1)
  * StepSize and DynamicStepSize (complex step sizes)
  * HMC.estimate_cov
The No-U-Turn sampler is bayeslim_amd.nuts (NUTS and TreeInfo on the tree-leaf kernels of csrc/nuts.hip); the two names here
stay stubs.
Dense mass matrices per key are bayeslim_amd.massmat (leapfrog, HMC and NUTS on the triangular kernels of csrc/massmat.hip).
RecycledHMC, StepSize, DynamicStepSize, pmask and estimate_cov are bayeslim_amd.recycled (on the fused kernel of csrc/recycle.hip);
the names here stay stubs.
"""
import math
import os
from datetime import datetime, timezone

import numpy as np
import torch

from . import _lib, utils
from .ops import _require_cuda, _stream, _ptr, _dtype_code
from .paramdict import ParamDict

# elements of one work-group and chunk of rime_hmc_step (256 lanes x 64 bytes), and the most work-groups of a launch
STEP_SPAN = {torch.float32: 4096, torch.float64: 2048}
STEP_MAXBLOCKS = 1024

_HMAT = ('sampler: %s must be None, a number or a real tensor of the shape of its parameter (a diagonal Cholesky factor); dense '
         'mass matrices (diag_mass=False) and the hmat operators of the reference (DenseMat, SolveMat, HierMat, SolveHierMat, '
         'DiagMat, ...) are not provided')


def _missing(what):
    raise NotImplementedError('sampler: %s of the reference is not provided' % what)


def _real_dtype(dtype):
    if dtype in (torch.float32, torch.complex64):
        return torch.float32
    if dtype in (torch.float64, torch.complex128):
        return torch.float64
    raise TypeError('sampler: float32 / float64 (or complex64 / complex128) parameters only, got %s' % dtype)


def _check_vectors(module, what, first, others, dtype_first=False):
    """
    The call layer of the flat-vector kernels (hmc_step here, nuts.leaf_open / leaf_close, massmat.project / drift): `first`, a
    contiguous real vector on the GPU, sets dtype, length and device, and every other vector that is given agrees with it.
    Returns (N, dtype code); raises in the words of `module`.  A dtype that is not provided is named after the operands have
    been judged, or before them with dtype_first (hmc_step's order).
    """
    _require_cuda(first)
    code = _dtype_code(_real_dtype(first.dtype)) if dtype_first else None
    N = first.numel()
    for t in others:
        if t is not None and (t.dtype != first.dtype or t.numel() != N or t.device != first.device or not t.is_contiguous()):
            raise ValueError('%s: contiguous vectors of %s [%d] on %s are needed' % (module, first.dtype, N, first.device))
    if first.is_complex() or not first.is_contiguous():
        raise ValueError('%s: %s takes contiguous real vectors (complex parameters as their interleaved views)' % (module, what))
    return N, (_dtype_code(_real_dtype(first.dtype)) if code is None else code)


def _check_out(module, out, device):
    """the three doubles (energy and the two projections) a kernel writes"""
    if out.dtype != torch.float64 or out.numel() < 3 or out.device != device or not out.is_contiguous():
        raise ValueError('%s: out must be a contiguous float64 tensor of three elements on %s' % (module, device))


def _workspace(need, device, ws=None):
    """ws if it holds at least `need` bytes (what a rime_*_workspace call answered), else a fresh workspace of that size"""
    if ws is None or ws.numel() * 8 < need:
        ws = torch.empty(int(need) // 8, dtype=torch.float64, device=device)
    return ws


def hmc_step(q, p, g, eps, c, kick, drift, energy=None, ws=None):
    """
    One launch of rime_hmc_step on flat real vectors (see include/rime_hip.h): q, p in place; g, eps, c may be None as the
    header allows; energy a float64 tensor of one element or None; ws the workspace for the energy (allocated if None).
    """
    N, code = _check_vectors('sampler', 'hmc_step', p, (q, g, eps, c), dtype_first=True)
    ws = None if energy is None else _workspace(_lib.lib.rime_hmc_workspace(N), p.device, ws)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib.rime_hmc_step(code, N, _ptr(q), _ptr(p), _ptr(g), _ptr(eps), _ptr(c), float(kick), float(drift),
                                          _ptr(energy), _ptr(ws), 0 if ws is None else ws.numel() * 8, _stream()), 'rime_hmc_step')


class _Layout:
    """
    Where every key lives in the flat real vector: offsets in real elements (even for a complex key, so that its slice can be
    viewed as complex; a gap of one element then holds zeros in every buffer and contributes nothing).
    """
    def __init__(self, x):
        self.tensor = isinstance(x, torch.Tensor)
        items = [(None, x)] if self.tensor else x.items()
        if len(items) == 0:
            raise ValueError('sampler: no parameters')
        first = items[0][1]
        self.on_gpu = all(v.is_cuda for _, v in items)
        self._items = items
        self.device, self.rdtype = first.device, _real_dtype(first.dtype)
        self.keys, self.slices, self.shapes, self.cplx = [], {}, {}, {}
        n = 0
        for k, v in items:
            if v.device != self.device or _real_dtype(v.dtype) != self.rdtype:
                raise ValueError('sampler: all parameters must share one device and one precision (%s on %s, %s on %s)'
                                 % (first.dtype, first.device, v.dtype, v.device))
            cp = v.is_complex()
            n += (n & 1) if cp else 0
            m = v.numel() * (2 if cp else 1)
            self.keys.append(k)
            self.slices[k], self.shapes[k], self.cplx[k] = slice(n, n + m), tuple(v.shape), cp
            n += m
        self.N = n

    def require_cuda(self):
        """the project's error for parameters that are not on the GPU (after the arguments have been judged)"""
        _require_cuda(*[v for _, v in self._items])
        self._items = None

    def new(self):
        return torch.zeros(self.N, dtype=self.rdtype, device=self.device)

    def view(self, buf, k):
        t = buf[self.slices[k]]
        if self.cplx[k]:
            t = torch.view_as_complex(t.reshape(-1, 2))
        return t.reshape(self.shapes[k])

    def views(self, buf):
        """the buffer as the caller's container: a ParamDict of views (or the one tensor)"""
        return self.view(buf, None) if self.tensor else ParamDict({k: self.view(buf, k) for k in self.keys})

    def pack(self, x, buf):
        """copy a container (same keys and shapes) into the buffer"""
        for k in self.keys:
            self.view(buf, k).copy_(x if self.tensor else x[k])
        return buf

    def unpack(self, buf, x):
        """copy the buffer back into a container (same keys and shapes)"""
        for k in self.keys:
            (x if self.tensor else x[k]).copy_(self.view(buf, k))

    def factor(self, val, what):
        """expand(val, what) as a launch takes it: None when the factor is 1 everywhere, a flat vector otherwise"""
        c = self.expand(val, what)
        if isinstance(c, float):
            c = None if c == 1.0 else torch.full((self.N,), c, dtype=self.rdtype, device=self.device)
        return c

    def classify(self, val, what):
        """
        Judge a step size or Cholesky factor -- None, a number, a real tensor, or a dict / ParamDict of those by key: returns
        (value per key, {key: float or None} for the keys whose value is one number or absent); raises for anything else.
        """
        per_key = {k: (val[k] if isinstance(val, (dict, ParamDict)) else val) for k in self.keys}
        scal = {}
        for k, v in per_key.items():
            if v is None:
                scal[k] = None
            elif isinstance(v, (int, float)):
                scal[k] = float(v)
            elif isinstance(v, torch.Tensor):
                if v.is_complex():
                    raise NotImplementedError('sampler: a complex %s (the reference\'s StepSize / complex masks) is not provided' % what)
                if v.numel() == 1:
                    scal[k] = float(v)
                elif tuple(v.shape) != self.shapes[k]:
                    raise NotImplementedError(_HMAT % what + ' [got shape %s for a parameter of shape %s]'
                                              % (tuple(v.shape), self.shapes[k]))
            else:
                raise NotImplementedError(_HMAT % what + ' [got %s]' % type(v).__name__)
        return per_key, scal

    def expand(self, val, what, fill=1.0):
        """val (see classify) as a flat vector, or a float when it is one number for every element, or None when it is absent
        everywhere; a key without a value is filled with `fill`"""
        per_key, scal = self.classify(val, what)
        if len(scal) == len(per_key) and len(set(scal.values())) == 1:
            return next(iter(scal.values()))
        out = torch.full((self.N,), fill, dtype=self.rdtype, device=self.device)
        for k, v in per_key.items():
            dst = out[self.slices[k]]
            if k in scal:
                dst.fill_(fill if scal[k] is None else scal[k])
            else:
                v = v.detach().to(device=self.device, dtype=self.rdtype).reshape(-1)
                dst.copy_(v.repeat_interleave(2) if self.cplx[k] else v)
        return out


class _Trajectory:
    """the flat buffers of one sampler or one leapfrog call, and the launches on them"""

    def __init__(self, layout, q=None, p=None):
        self.lay = layout
        self.q = layout.new() if q is None else q
        self.p = layout.new() if p is None else p
        self.g = layout.new()
        self.qv, self.pv = layout.views(self.q), layout.views(self.p)
        self.energy = torch.zeros(1, dtype=torch.float64, device=layout.device)
        self.ws = _workspace(_lib.lib.rime_hmc_workspace(layout.N), layout.device)
        self.launches = 0

    def stage(self, eps, c, kick, drift, energy=False):
        """one launch; eps a float (folded into kick and drift) or a flat vector; returns the kinetic energy if asked"""
        vec = isinstance(eps, torch.Tensor)
        s = 1.0 if vec else float(eps)
        hmc_step(self.q if drift else None, self.p, self.g if kick else None, eps if vec else None, c, kick * s, drift * s,
                 self.energy if energy else None, self.ws)
        self.launches += 1
        return float(self.energy) if energy else None

    def kinetic(self, c):
        """1/2 sum (c p)^2 of the momentum buffer: the energy-only pass"""
        return self.stage(1.0, c, 0.0, 0.0, energy=True)

    def set_grad(self, grad):
        self.lay.pack(grad, self.g)

    def run(self, dUdq, eps, c, N, dUdq0=None, states=None, energy=False):
        """N leapfrog steps in place on the buffers; dUdq(q, Ucache=[]) is called on the views of the position buffer"""
        def gradient():
            cache = []
            grad = dUdq(self.qv, Ucache=cache)
            self.set_grad(grad)
            return grad, (cache[-1] if cache else None)

        def clone(v):
            return v.clone()

        U = None
        if dUdq0 is None:
            dUdq0, U = gradient()
        else:
            self.set_grad(dUdq0)
        if states is not None:
            states.append((clone(self.qv), clone(self.pv), U, dUdq0))
        if N < 1:
            return None
        self.stage(eps, c, 0.5, 1.0)
        for _ in range(N - 1):
            grad, U = gradient()
            if states is not None:
                # before the launch that kicks AND drifts on: the position of this time, the momentum half a kick on
                half = self.lay.views((0.5 * (eps if isinstance(eps, torch.Tensor) else float(eps))) * self.g)
                states.append((clone(self.qv), self.pv - half, U, grad))
            self.stage(eps, c, 1.0, 1.0)
        grad, U = gradient()
        K = self.stage(eps, c, 0.5, 0.0, energy=energy)
        if states is not None:
            states.append((clone(self.qv), clone(self.pv), U, grad))
        return K


def _check_diag(diag_mass, keys):
    flags = diag_mass.values() if isinstance(diag_mass, (dict, ParamDict)) else [diag_mass]
    if not all(bool(f) for f in flags):
        raise NotImplementedError('sampler: diag_mass=False (a dense mass matrix, the reference\'s DenseMat / SolveMat / HierMat '
                                  'path) is not provided; only identity and diagonal mass matrices are')


def leapfrog(q, p, dUdq, eps, N, cov_L=None, diag_mass=True, dUdq0=None, states=None):
    """
    N leapfrog steps of position q and momentum p, in place (reference sampler.leapfrog), on the fused kernel: N + 1 launches.

    q, p : tensors or ParamDicts on the GPU, one precision;  dUdq : callable (q, Ucache=[]) -> gradient of the potential at q
    in the container type of q, appending the potential to Ucache if it wants it recorded;  eps : number, real tensor or
    ParamDict of those (per key or per element);  cov_L : None, number, real tensor or ParamDict of those: the diagonal
    Cholesky factor of the covariance (inverse mass), dq = eps cov_L^2 p;  dUdq0 : the gradient at the input q if known;
    states : list that receives (q, p, U, gradient) at the start and after every step, p at the position's time.
    Returns (q, p).
    """
    if isinstance(q, ParamDict) != isinstance(p, ParamDict):
        raise TypeError('sampler.leapfrog: q and p must both be tensors or both be ParamDicts')
    _check_diag(diag_mass, None)
    lay = _Layout(q)
    lay.classify(eps, 'eps')
    lay.classify(cov_L, 'cov_L')
    _Layout(p).require_cuda()
    lay.require_cuda()
    direct = lay.tensor and q.is_contiguous() and p.is_contiguous() and not q.requires_grad and not p.requires_grad \
        and p.dtype == q.dtype and p.shape == q.shape
    if direct:                                      # the caller's own storage is the flat buffer
        real = lambda t: torch.view_as_real(t).reshape(-1) if t.is_complex() else t.reshape(-1)
        traj = _Trajectory(lay, real(q), real(p))
    else:
        traj = _Trajectory(lay)
        with torch.no_grad():
            lay.pack(q, traj.q)
            lay.pack(p, traj.p)
    e = lay.expand(eps, 'eps')
    if e is None:
        raise ValueError('sampler.leapfrog: eps is None')
    c = lay.factor(cov_L, 'cov_L')
    with torch.no_grad():
        traj.run(dUdq, e, c, N, dUdq0=dUdq0, states=states)
        if not direct:
            lay.unpack(traj.q, q)
            lay.unpack(traj.p, p)
    return q, p


class SamplerBase:
    """
    The chain bookkeeping of every sampler (reference SamplerBase): x the current position (ParamDict), chain a dict of lists
    of numpy arrays per key, Uchain the potentials, _acceptances, accept_ratio.
    """
    def __init__(self, x0):
        self.x = ParamDict({k: v.detach().clone() for k, v in x0.items()})
        self.accept_ratio = 1.0
        self._acceptances = []
        self.chain = {k: [] for k in x0.keys()}
        self.Uchain = []
        self._lists = ['_acceptances', 'Uchain']          # attributes that are lists: wrapped on write, unwrapped on load

    def step(self):
        """one move: update self.x and return (accept, probability); a subclass provides it"""
        raise NotImplementedError

    def append_chain(self, q, U=None):
        for k in q.keys():
            self.chain[k].append(utils.tensor2numpy(q[k], clone=True))
        self.Uchain.append(U)

    def sample(self, Nsample, Ncheck=None, outfile=None, description=''):
        """Nsample steps appended to the chain; every Ncheck-th step the chain is written to outfile (npz)"""
        for i in range(Nsample):
            accept, prob = self.step()
            self._acceptances.append(utils.tensor2numpy(accept))
            self.append_chain(self.x, U=self._U)
            if Ncheck is not None and i > 0 and i % Ncheck == 0:
                assert outfile is not None
                self.write_chain(outfile, overwrite=True, description=description)
        self.accept_ratio = sum(self._acceptances) / len(self._acceptances)

    def get_chain(self, keys=None):
        keys = list(self.chain.keys()) if keys is None else ([keys] if isinstance(keys, str) else keys)
        return {k: torch.as_tensor(np.asarray(self.chain[k])) for k in keys}

    def _write_chain(self, outfile, attrs=(), overwrite=False, description=''):
        if os.path.exists(outfile) and not overwrite:
            print('{} exists, not overwriting...'.format(outfile))
            return
        if len(self._acceptances):
            self.accept_ratio = sum(self._acceptances) / len(self._acceptances)
        out = {}
        for attr in ['chain', '_acceptances', 'accept_ratio', 'x', 'Uchain'] + list(attrs):
            val = getattr(self, attr)
            if attr == 'x':
                val = val.push('cpu', inplace=False)
            out[attr] = np.empty((), dtype=object)               # one pickled object per attribute, whatever its type
            out[attr][()] = {attr: val} if attr in self._lists else val
        out['description'] = 'Written UTC: {}\n{}\n{}'.format(datetime.now(timezone.utc).replace(tzinfo=None), '-' * 40, description)
        np.savez(outfile, **out)

    def write_chain(self, outfile, overwrite=False, description=''):
        """write chain, _acceptances, accept_ratio, x (on the CPU) and Uchain to an npz file"""
        self._write_chain(outfile, overwrite=overwrite, description=description)

    def load_chain(self, infile):
        """attach everything write_chain wrote (x comes back on the CPU: push it where it is needed)"""
        with np.load(infile, allow_pickle=True) as f:
            for key in f.files:
                if key == 'description':
                    continue
                val = f[key].item()
                setattr(self, key, val[key] if key in self._lists else val)

    def clear_chain(self, N=None):
        """drop the oldest N entries (default: all)"""
        Nclear = len(self.Uchain) if N is None else N
        for k in self.chain:
            self.chain[k] = self.chain[k][Nclear:]
        self.Uchain = self.Uchain[Nclear:]
        if hasattr(self, '_divergences'):
            self._divergences = [(d[0] - Nclear,) + tuple(d[1:]) for d in self._divergences]


class HMC(SamplerBase):
    """
    Hamiltonian Monte Carlo with a fixed step size and trajectory length (reference sampler.HMC; Neal 2011), identity or
    diagonal mass.

    potential_fn(x) -> (U, gradient ParamDict) for a ParamDict x;  x0 : ParamDict on the GPU;  eps : number, real tensor or
    ParamDict (per key or per element);  cov_L / hess_L : ParamDicts (or dicts) of the diagonal Cholesky factors of the
    covariance / of the mass matrix, tensors of the parameters' shapes, numbers or None per key; given one, the other is its
    element-wise reciprocal;  Nstep : leapfrog steps per move;  pdist : dict of callables returning the base momentum per
    key (default: unit Gaussian by torch.randn on the device);  dHmax : a move whose Hamiltonian grows by more is divergent:
    it is refused and the sampler restarts from a random entry of the chain;  U0 : the potential at x0 if known.

    The Metropolis draw is np.random.rand() and the restart index np.random.randint, so a seeded numpy generator reproduces
    the reference's decisions.  After step(), `_last` holds K_start, H_start and H_end of the move as floats.
    """
    def __init__(self, potential_fn, x0, eps, cov_L=None, hess_L=None, diag_mass=True, Nstep=10, pdist=None, pmask=None,
                 dHmax=1000, record_divergences=False, U0=None):
        if pmask is not None:
            _missing('pmask (momentum masks)')
        if not isinstance(x0, ParamDict):
            raise TypeError('sampler.HMC: x0 must be a ParamDict')
        self._judge_diag(diag_mass)
        self._lay = _Layout(x0)
        self._judge_mass(eps, cov_L, hess_L, diag_mass)
        self._lay.require_cuda()                                 # the arguments are judged first, then the device
        super().__init__(x0)
        self._lists += ['_divergences']
        self._traj = self._new_trajectory()
        self.potential_fn = potential_fn
        self.fn_evals = 0
        self.Nstep = Nstep
        self.dHmax = dHmax
        self.record_divergences = record_divergences
        self._divergences = []                                   # [(chain length, final x, final p), ...]
        if U0 is None:
            self._U, self._gradU = self.potential_fn(self.x)
        else:
            self._U, self._gradU = U0, None
        self.p = None
        self.eps = eps
        self.pdist = pdist
        self.pmask = None
        self._last = {}
        self.set_chol(cov_L=cov_L, hess_L=hess_L, diag_mass=diag_mass)

    # ------------------------------------------------------------------ what a subclass with another mass replaces (massmat)
    def _judge_diag(self, diag_mass):
        _check_diag(diag_mass, None)

    def _judge_mass(self, eps, cov_L, hess_L, diag_mass):
        for L, what in ((eps, 'eps'), (cov_L, 'cov_L'), (hess_L, 'hess_L')):
            if isinstance(L, (dict, ParamDict)) or what == 'eps':
                self._lay.classify(L, what)
            elif L is not None:
                raise NotImplementedError(_HMAT % what + ' [got %s]' % type(L).__name__)

    def _new_trajectory(self):
        return _Trajectory(self._lay)

    # ------------------------------------------------------------------ step size and mass
    @property
    def eps(self):
        return self._eps

    @eps.setter
    def eps(self, eps):
        if isinstance(eps, torch.Tensor):
            eps = ParamDict({k: eps for k in self._lay.keys})
        flat = self._lay.expand(eps, 'eps')
        if flat is None:
            raise ValueError('sampler.HMC: eps is None')
        self._eps, self._eps_flat = eps, flat

    def set_chol(self, cov_L=None, hess_L=None, diag_mass=True):
        """
        Set the Cholesky factors of the diagonal covariance (cov_L: scales the drift and the kinetic energy) and of the
        diagonal mass matrix (hess_L: scales the drawn momenta).  Given one, the other is 1 / it; given neither, unit mass.
        logdetM = 2 sum log hess_L, which K() adds to the kinetic energy as the reference does.
        """
        _check_diag(diag_mass, self._lay.keys)
        keys = self._lay.keys

        def per_key(L, what):
            if L is None:
                return None
            if not isinstance(L, (dict, ParamDict)):
                raise NotImplementedError(_HMAT % what + ' [got %s]' % type(L).__name__)
            self._lay.expand(L, what)                             # validates types and shapes
            return {k: (torch.as_tensor(L[k], dtype=self._lay.rdtype, device=self._lay.device) if L[k] is not None else None)
                    for k in keys}

        cov_L, hess_L = per_key(cov_L, 'cov_L'), per_key(hess_L, 'hess_L')
        recip = lambda L: {k: (None if v is None else torch.true_divide(1, v)) for k, v in L.items()}
        if cov_L is not None and hess_L is None:
            hess_L = recip(cov_L)
        if hess_L is not None and cov_L is None:
            cov_L = recip(hess_L)
        if cov_L is None:
            cov_L, hess_L = {k: None for k in keys}, {k: None for k in keys}
        self.cov_L, self.hess_L = cov_L, hess_L
        self.diag_mass = {k: True for k in keys}
        self._c = self._lay.factor(cov_L, 'cov_L')
        self.logdetM = torch.zeros((), dtype=torch.float64, device=self._lay.device)
        for k in keys:
            if hess_L[k] is not None:
                self.logdetM += 2 * torch.sum(torch.log(hess_L[k].double()))
        self._logdetM = float(self.logdetM)

    # ------------------------------------------------------------------ energies and gradients
    @torch.no_grad()
    def K(self, p):
        """kinetic energy 1/2 p^T C p + logdetM of a momentum ParamDict (or tensor: unit mass), as a float64 tensor"""
        if isinstance(p, torch.Tensor):
            _require_cuda(p)
            flat = torch.view_as_real(p.contiguous()).reshape(-1) if p.is_complex() else p.contiguous().reshape(-1)
            e = torch.zeros(1, dtype=torch.float64, device=p.device)
            hmc_step(None, flat.detach(), None, None, None, 0.0, 0.0, e)
            return e[0] + self.logdetM
        tr = self._traj
        if p is not tr.pv:
            tr.lay.pack(p, tr.p)
        return torch.tensor(tr.kinetic(self._c), dtype=torch.float64) + self._logdetM

    def is_divergent(self, H_start, H_end):
        return (H_end - H_start) > self.dHmax

    def dUdx(self, x, Ucache=None, **kwargs):
        """potential and gradient at x: sets _U and _gradU, counts fn_evals, appends U to Ucache, returns the gradient"""
        self._U, self._gradU = self.potential_fn(x)
        self.fn_evals += 1
        if Ucache is not None:
            Ucache.append(self._U)
        return self._gradU

    def draw_momentum(self):
        """
        Fresh momenta in the sampler's momentum buffer: per key pdist[k]() or a unit Gaussian (torch.randn on the device),
        times hess_L[k].  Returns the ParamDict of views of that buffer.
        """
        tr = self._traj
        for k in tr.lay.keys:
            x = self.x[k]
            m = self.pdist[k]() if self.pdist is not None else torch.randn(x.numel(), device=x.device, dtype=x.dtype)
            m = m.reshape(x.shape)
            L = self.hess_L[k]
            tr.pv[k].copy_(m if L is None else L * m)
        return tr.pv

    # ------------------------------------------------------------------ the move
    @torch.no_grad()
    def step(self, sample_p=True):
        """
        One HMC move with its Metropolis decision; sample_p=False starts from the stored momentum self.p instead of a fresh
        draw.  Returns (accept, prob) as 0-d tensors.
        """
        tr = self._traj
        tr.lay.pack(self.x, tr.q)
        if sample_p:
            self.draw_momentum()
        else:
            tr.lay.pack(self.p, tr.p)
        K_start = tr.kinetic(self._c) + self._logdetM

        with torch.enable_grad():
            self.dUdx(tr.qv)
        U_start, dUdq0 = self._U, self._gradU
        H_start = K_start + float(U_start)

        def dUdq(q, Ucache=None):
            with torch.enable_grad():
                return self.dUdx(q, Ucache=Ucache)

        K_end = tr.run(dUdq, self._eps_flat, self._c, self.Nstep, dUdq0=dUdq0, energy=True)
        if K_end is None:                                        # Nstep = 0: nothing moved
            K_end = tr.kinetic(self._c)
        H_end = K_end + self._logdetM + float(self._U)
        self._last = dict(K_start=K_start, H_start=H_start, H_end=H_end)

        restore = False
        if self.is_divergent(H_start, H_end):
            Nchain = len(self.Uchain)
            if self.record_divergences:
                self._divergences.append((Nchain, tr.qv.clone(), tr.pv.clone()))
            if Nchain > 0:                                       # restart from a random entry of the chain
                i = np.random.randint(0, Nchain)
                self._U = self.Uchain[i]
                self.x = ParamDict({k: torch.as_tensor(self.chain[k][i], device=self.x[k].device) for k in self.x})
            restore = True
            accept, prob = False, 0.0
        else:
            d = H_start - H_end
            prob = 1.0 if d >= 0 else math.exp(d) if d == d else float('nan')
            accept = bool(math.isfinite(H_end) and (np.random.rand() < prob))
            if accept:
                self.x = tr.qv.clone()
                self.p = tr.pv.clone()
            else:
                self._U, self._gradU = U_start, dUdq0
                restore = True
        if restore and isinstance(self.potential_fn, Potential):
            self.potential_fn.prob.update(self.x)                # the model holds the position the chain holds
        return torch.tensor(accept), torch.tensor(prob, dtype=torch.float64)

    def dual_averaging(self, Nadapt, target=0.8, gamma=0.05, t0=10.0, kappa=0.75):
        """
        Nadapt moves that adapt the step size by the dual averaging of Hoffman & Gelman (2014), eqn 6, starting from and
        replacing self.eps.  As in the reference, eps is left at the last iterate exp(log eps_i), not at the running average.
        """
        as_dict = isinstance(self._eps, ParamDict)
        mu = (10 * self._eps).operator(torch.log) if as_dict else math.log(10 * float(self._eps))
        h_bar = 0.0
        for i in range(1, Nadapt + 1):
            _, prob = self.step()
            eta = 1.0 / (i + t0)
            h_bar = (1 - eta) * h_bar + eta * (target - float(prob))
            log_eps = mu - h_bar * math.sqrt(i) / gamma
            self.eps = log_eps.operator(torch.exp) if as_dict else math.exp(log_eps)

    def estimate_cov(self, *args, **kwargs):
        _missing('HMC.estimate_cov')

    def write_chain(self, outfile, overwrite=False, description=''):
        """as SamplerBase.write_chain, plus fn_evals and the recorded divergences"""
        self._write_chain(outfile, overwrite=overwrite, attrs=['fn_evals', '_divergences'], description=description)


class RecycledHMC(HMC):
    def __init__(self, *args, **kwargs):
        _missing('RecycledHMC')


class TreeInfo:
    def __init__(self, *args, **kwargs):
        _missing('TreeInfo (NUTS)')


class NUTS(HMC):
    def __init__(self, *args, **kwargs):
        _missing('NUTS (with TreeInfo)')


class StepSize(ParamDict):
    def __init__(self, *args, **kwargs):
        _missing('StepSize')


class DynamicStepSize(StepSize):
    def __init__(self, *args, **kwargs):
        _missing('DynamicStepSize')


class Potential(utils.Module):
    """
    The potential of a posterior: the negative log posterior of an optim.LogProb and its gradient (reference
    sampler.Potential).  prob : optim.LogProb;  param_name : the attribute of prob a tensor argument replaces.
    """
    def __init__(self, prob, param_name=None):
        super().__init__()
        self.prob = prob
        self.param_name = param_name

    def forward(self, x=None, **kwargs):
        """
        x : ParamDict keyed by the names of prob's parameters ('model.sky.params', 'main_params', ...), or a tensor for
        prob[param_name], or None to evaluate where the model stands.  Returns (U, ParamDict of cloned gradients).
        """
        if x is not None:
            if isinstance(x, ParamDict):
                self.prob.update(x)
            else:
                self.prob[self.param_name] = torch.as_tensor(x)
        self.prob.zero_grad()
        U = self.prob.closure()
        return U, ParamDict({k: self.prob[k].grad.clone() for k in self.prob.named_params})

    def __call__(self, x=None, **kwargs):
        return self.forward(x=x, **kwargs)


def hoffman_uturn(q_minus, q_plus, p_minus, p_plus):
    """
    The no-U-turn criterion of Hoffman & Gelman (2014): True when the span q_plus - q_minus has a negative projection on the
    momentum at either end.  Tensors or ParamDicts; two dot products in plain torch.
    """
    if isinstance(q_minus, torch.Tensor):
        q_minus, q_plus, p_minus, p_plus = ({'_': t} for t in (q_minus, q_plus, p_minus, p_plus))
    lo = hi = 0
    for k in q_minus:
        span = (q_plus[k] - q_minus[k]).conj().ravel()
        lo = lo + (span @ p_minus[k].ravel()).real
        hi = hi + (span @ p_plus[k].ravel()).real
    return bool(lo < 0) or bool(hi < 0)
