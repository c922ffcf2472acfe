"""
Dense-mass Hamiltonian Monte Carlo and No-U-Turn sampling on the triangular kernels of csrc/massmat.hip: the counterpart of the
reference's sampler.HMC.set_chol, HMC.K, HMC.draw_momentum and leapfrog.pos_step (sampler.py:260-450, 489-546, 1516-1554) for a
dense lower-triangular Cholesky factor per parameter key.  sampler.HMC, sampler.leapfrog and nuts.NUTS keep refusing
diag_mass=False in their own words; the dense-mass samplers live here: massmat.leapfrog, massmat.HMC, massmat.NUTS.

With cov_L[k] = Lc (covariance C = Lc Lc^T) a leapfrog stage needs z = Lc^T p, dq = Lc z and K = 1/2 z^T z.  A stage is TWO
launches over the flat parameter vector of sampler._Layout, whatever the number of keys:
  rime_mass_project   the momentum kick out of place (two momentum buffers alternate) and z = Lc^T p on the dense keys, c * p on
                      the others
  rime_mass_drift     q += eps Lc z on the dense keys, eps c z on the others, and on request the kinetic energy and the two
                      no-U-turn projections in the fixed summation order of rime_hmc_step
so a trajectory of N steps is 2 (N + 1) launches, a NUTS leaf four (project + drift from the read-only edge state, the gradient,
project with the second half kick into a fresh buffer, drift with drift = 0 for the energy and the projections) and one readback
of three doubles, and K(p) two.  The dense keys are a device table of blocks (BlockTable): per key the factor, its leading
dimension, its offset in the flat vector and nrhs (1 for a real key; 2 for a complex key, whose interleaved real view takes the
same real factor on both components, as the reference applies a real factor to .real and .imag).

set_chol follows the reference: a dense cov_L[k] without hess_L[k] draws the momentum by one triangular solve Lc^T p = p0 per
move (torch.linalg.solve_triangular) and adds nothing to logdetM (the reference's implicit SolveMat adds nothing); with both,
p = hess_L[k] p0 per component and logdetM += 2 sum log diag hess_L[k].  A key with diag_mass[k] true takes what sampler.HMC takes.

Not provided (each raises NotImplementedError naming what is missing):
  * a dense hess_L[k] without cov_L[k] (the reference's implicit-solve covariance: two triangular solves per stage)
  * any hmat operator but DenseMat and TriangMat as a mass: SolveMat, HierMat, SolveHierMat, SparseMat, PartitionedMat, ...
  * a complex factor, a factor of the wrong shape
  * pmask; RecycledHMC, StepSize and DynamicStepSize stay where they are (sampler)
There is no CPU path.
"""
import numpy as np
import torch

from . import _lib, hmat, nuts, sampler
from .ops import _require_cuda, _stream, _ptr
from .paramdict import ParamDict

# rows of a strip of the L z kernel, columns of a strip of the L^T p kernel (8 x 16 bytes), per precision
LOWER_ROWS = 4
UPPER_COLS = {torch.float32: 32, torch.float64: 16}

_OPERATOR = ('massmat: %s[%r] must be a real (n, n) tensor, an hmat.DenseMat or an hmat.TriangMat holding the lower-triangular '
             'Cholesky factor; the other hmat operators of the reference (SolveMat, HierMat, SolveHierMat, SparseMat, '
             'PartitionedMat, DiagMat, ...) are not provided as a dense mass')


def _flags(diag_mass, keys):
    if isinstance(diag_mass, (dict, ParamDict)):
        return {k: bool(diag_mass[k]) for k in keys}
    return {k: bool(diag_mass) for k in keys}


def _per_key(val, keys, what):
    if val is None:
        return {k: None for k in keys}
    if isinstance(val, (dict, ParamDict)):
        return {k: val[k] for k in keys}
    if len(keys) == 1:
        return {keys[0]: val}
    raise NotImplementedError('massmat: %s must be a dict or ParamDict by key [got %s]' % (what, type(val).__name__))


def _dense(v, k, n, what):
    """the real (n, n) factor of key k as a tensor (None stays None); raises for anything else"""
    if v is None:
        return None
    if isinstance(v, hmat.TriangMat):
        if not v.lower:
            raise NotImplementedError('massmat: %s[%r] is an upper-triangular TriangMat; the lower-triangular factor is needed' % (what, k))
        v = v.to_dense()
    elif isinstance(v, hmat.DenseMat):
        v = v.H
    elif not isinstance(v, torch.Tensor):
        raise NotImplementedError(_OPERATOR % (what, k) + ' [got %s]' % type(v).__name__)
    if v.is_complex():
        raise NotImplementedError('massmat: a complex %s[%r] is not provided (a real factor acts on both components of a complex key)'
                                  % (what, k))
    if tuple(v.shape) != (n, n):
        raise NotImplementedError('massmat: %s[%r] has shape %s; a dense factor of a parameter of %d elements is (%d, %d)'
                                  % (what, k, tuple(v.shape), n, n, n))
    return v


def make_table(blocks, N, dtype, device):
    """
    The device table of rime_mass_block (include/rime_hip.h) of blocks = [(L, off, nrhs), ...]: L a real 2-d tensor of `dtype` on
    `device` whose rows are contiguous (stride (ld, 1), ld >= n), off the first flat element, nrhs 1 or 2.  Validates n, ld, off,
    nrhs and that the blocks do not overlap; returns (int64 tensor [nblocks, 8] or None, the tensors it points into).
    """
    rows, spans = [], []
    for L, off, nrhs in blocks:
        if L.ndim != 2 or L.shape[0] != L.shape[1] or L.shape[0] < 1 or L.dtype != dtype or L.is_complex():
            raise ValueError('massmat: a block is a real square matrix of %s, got %s %s' % (dtype, tuple(L.shape), L.dtype))
        n = L.shape[0]
        ld = L.stride(0) if n > 1 else max(L.stride(0), 1)
        if (n > 1 and L.stride(1) != 1) or ld < n:
            raise ValueError('massmat: the rows of a block must be contiguous with a leading dimension >= n (strides %s)' % (L.stride(),))
        if nrhs not in (1, 2):
            raise ValueError('massmat: nrhs must be 1 or 2, got %r' % (nrhs,))
        if off < 0 or off + n * nrhs > N:
            raise ValueError('massmat: a block of %d x %d elements at offset %d does not fit a vector of %d' % (n, nrhs, off, N))
        spans.append((off, off + n * nrhs))
        rows.append([L.data_ptr(), ld, off, n | (nrhs << 32), 0, 0, 0, 0])
    spans.sort()
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        if b0 < a1:
            raise ValueError('massmat: blocks overlap (elements %d ... %d and %d ... %d)' % (a0, a1 - 1, b0, b1 - 1))
    if not rows:
        return None, []
    _require_cuda(*[L for L, _, _ in blocks])
    return torch.tensor(rows, dtype=torch.int64).to(device), [L for L, _, _ in blocks]


class BlockTable:
    """
    The dense keys of a sampler._Layout as blocks: entries = [dict(key, n, ld, off, nrhs), ...] in the order of the layout, `c` what
    sampler._Layout.expand makes of the diagonal keys' factors (ones on the dense keys), `dense` {key: factor} in the layout's
    precision.  Judged on construction (on any device); table() builds the device table.
    """
    def __init__(self, lay, cov_L, diag_mass, what='cov_L'):
        self.lay, self.flags = lay, _flags(diag_mass, lay.keys)
        per_key = _per_key(cov_L, lay.keys, what)
        self.dense, self.entries, diag = {}, [], {}
        for k in lay.keys:
            n = int(np.prod(lay.shapes[k], dtype=np.int64))
            if self.flags[k]:
                diag[k] = per_key[k]
                continue
            diag[k] = None
            L = _dense(per_key[k], k, n, what)
            if L is None:                                            # a dense key without a factor: unit mass
                continue
            L = L.detach().to(device=lay.device, dtype=lay.rdtype).contiguous()
            self.dense[k] = L
            self.entries.append(dict(key=k, n=n, ld=L.stride(0) if n > 1 else 1, off=lay.slices[k].start, nrhs=2 if lay.cplx[k] else 1))
        lay.classify(diag, what)
        self._diag, self._what, self._table = diag, what, None

    def diagonal(self):
        """the flat diagonal factor (None: ones everywhere)"""
        return self.lay.factor(self._diag, self._what)

    def table(self):
        if self._table is None:
            self._table = make_table([(self.dense[e['key']], e['off'], e['nrhs']) for e in self.entries], self.lay.N, self.lay.rdtype,
                                     self.lay.device)
        return self._table[0]

    def __len__(self):
        return len(self.entries)


def project(table, p_in, g, eps, c, kick, p_out, z):
    """one call of rime_mass_project on flat real vectors (see include/rime_hip.h); table from make_table or None"""
    N, code = sampler._check_vectors('massmat', 'project', p_in, (g, eps, c, p_out, z))
    with torch.cuda.device(p_in.device):
        _lib.check(_lib.lib.rime_mass_project(code, N, _ptr(table), 0 if table is None else table.shape[0], _ptr(p_in), _ptr(g),
                                              _ptr(eps), _ptr(c), float(kick), _ptr(p_out), _ptr(z), _stream()), 'rime_mass_project')


def drift(table, z, q_in, eps, c, drift, q_out, p=None, q_far=None, p_far=None, out=None, ws=None):
    """one call of rime_mass_drift on flat real vectors (see include/rime_hip.h); out a float64 tensor of three elements or None"""
    N, code = sampler._check_vectors('massmat', 'drift', z, (q_in, eps, c, q_out, p, q_far, p_far))
    if out is None:
        ws = None
    else:
        sampler._check_out('massmat', out, z.device)
        ws = sampler._workspace(_lib.lib.rime_mass_workspace(N), z.device, ws)
    with torch.cuda.device(z.device):
        _lib.check(_lib.lib.rime_mass_drift(code, N, _ptr(table), 0 if table is None else table.shape[0], _ptr(z), _ptr(q_in), _ptr(eps),
                                            _ptr(c), float(drift), _ptr(q_out), _ptr(p), _ptr(q_far), _ptr(p_far), _ptr(out),
                                            _ptr(ws), 0 if ws is None else ws.numel() * 8, _stream()), 'rime_mass_drift')


class _Trajectory(sampler._Trajectory):
    """sampler._Trajectory on the two launches of this module: a second momentum buffer, the projected momentum z, three sums"""

    def __init__(self, layout, owner):
        super().__init__(layout)
        self.owner = owner                                        # holds _blocks (a BlockTable), set before the first stage
        self.p2, self.z = layout.new(), layout.new()
        self.out = torch.zeros(3, dtype=torch.float64, device=layout.device)
        self.ws = sampler._workspace(_lib.lib.rime_mass_workspace(layout.N), layout.device)

    def stage(self, eps, c, kick, drift_, energy=False):
        """two launches; eps a float (folded into kick and drift) or a flat vector; returns the kinetic energy if asked"""
        vec = isinstance(eps, torch.Tensor)
        s = 1.0 if vec else float(eps)
        table, e = self.owner._blocks.table(), (eps if vec else None)
        if kick:
            project(table, self.p, self.g, e, c, kick * s, self.p2, self.z)
            self.p, self.p2 = self.p2, self.p
            self.pv = self.lay.views(self.p)
        else:
            project(table, self.p, None, None, c, 0.0, None, self.z)
        q = self.q if drift_ else None
        drift(table, self.z, q, e, c, drift_ * s, q, out=self.out if energy else None, ws=self.ws)
        self.launches += 2
        return float(self.out[0]) if energy else None


class _Holder:
    def __init__(self, blocks):
        self._blocks = blocks


def leapfrog(q, p, dUdq, eps, N, cov_L=None, diag_mass=True, dUdq0=None, states=None):
    """
    N leapfrog steps of position q and momentum p, in place (reference sampler.leapfrog), with a dense or diagonal Cholesky factor
    of the covariance per key: 2 (N + 1) launches.  Arguments as sampler.leapfrog; cov_L[k] of a key with diag_mass[k] false is a
    real (n, n) lower-triangular tensor (or an hmat.DenseMat / TriangMat of one), n the key's numel; for tensors q, p, cov_L and
    diag_mass are the tensor's own.  Returns (q, p).
    """
    if isinstance(q, ParamDict) != isinstance(p, ParamDict):
        raise TypeError('massmat.leapfrog: q and p must both be tensors or both be ParamDicts')
    lay = sampler._Layout(q)
    lay.classify(eps, 'eps')
    blocks = BlockTable(lay, cov_L, diag_mass)
    sampler._Layout(p).require_cuda()
    lay.require_cuda()
    traj = _Trajectory(lay, _Holder(blocks))
    e = lay.expand(eps, 'eps')
    if e is None:
        raise ValueError('massmat.leapfrog: eps is None')
    with torch.no_grad():
        lay.pack(q, traj.q)
        lay.pack(p, traj.p)
        traj.run(dUdq, e, blocks.diagonal(), N, dUdq0=dUdq0, states=states)
        lay.unpack(traj.q, q)
        lay.unpack(traj.p, p)
    return q, p


class _DenseMass:
    """what massmat.HMC and massmat.NUTS put in front of their parents: the judging of the mass, the trajectory, set_chol, the draw"""

    def _judge_diag(self, diag_mass):
        pass

    def _judge_mass(self, eps, cov_L, hess_L, diag_mass):
        lay = self._lay
        lay.classify(eps, 'eps')
        self._judge_chol(cov_L, hess_L, diag_mass)

    def _judge_chol(self, cov_L, hess_L, diag_mass):
        lay = self._lay
        for L, what in ((cov_L, 'cov_L'), (hess_L, 'hess_L')):
            if L is not None and not isinstance(L, (dict, ParamDict)):
                raise NotImplementedError('massmat: %s must be a dict or ParamDict by key [got %s]' % (what, type(L).__name__))
        cov, hess = BlockTable(lay, cov_L, diag_mass, 'cov_L'), BlockTable(lay, hess_L, diag_mass, 'hess_L')
        for k in hess.dense:
            if k not in cov.dense:
                raise NotImplementedError('massmat: a dense hess_L[%r] without cov_L[%r] (the reference\'s implicit-solve covariance: two '
                                          'triangular solves per stage) is not provided; pass the Cholesky factor of the covariance' % (k, k))
        return cov, hess

    def _new_trajectory(self):
        return _Trajectory(self._lay, self)

    def set_chol(self, cov_L=None, hess_L=None, diag_mass=True):
        """
        Set the Cholesky factors of the covariance (cov_L: the drift and the kinetic energy) and of the mass matrix (hess_L: the
        drawn momenta), per key dense (diag_mass[k] false: real (n, n) lower-triangular) or diagonal (as sampler.HMC.set_chol).
        A dense cov_L[k] alone: the momentum is drawn by solving cov_L[k]^T p = p0, and the key adds nothing to logdetM.
        """
        lay, keys = self._lay, self._lay.keys
        cov, hess = self._judge_chol(cov_L, hess_L, diag_mass)
        dev = dict(dtype=lay.rdtype, device=lay.device)
        as_t = lambda v: None if v is None else torch.as_tensor(v, **dev)
        cd, hd = {k: as_t(cov._diag[k]) for k in keys}, {k: as_t(hess._diag[k]) for k in keys}
        recip = lambda v: None if v is None else torch.true_divide(1, v)
        self.cov_L, self.hess_L = {}, {}
        for k in keys:
            if k in cov.dense:
                self.cov_L[k], self.hess_L[k] = cov.dense[k], hess.dense.get(k)
            else:
                c, h = cd[k], hd[k]
                self.cov_L[k] = c if c is not None else recip(h)
                self.hess_L[k] = h if h is not None else recip(c)
        self.diag_mass = {k: k not in cov.dense for k in keys}
        # the diagonal factor of the launches: the covariance's, with the reciprocal of a lone hess_L
        cov._diag = {k: (self.cov_L[k] if self.diag_mass[k] else None) for k in keys}
        self._blocks, self._c = cov, cov.diagonal()
        self.logdetM = torch.zeros((), dtype=torch.float64, device=lay.device)
        for k in keys:
            h = self.hess_L[k]
            if h is not None:
                self.logdetM += 2 * torch.sum(torch.log((h if self.diag_mass[k] else h.diagonal()).double()))
        self._logdetM = float(self.logdetM)

    def draw_momentum(self):
        """
        Fresh momenta in the sampler's momentum buffer: per key pdist[k]() or a unit Gaussian, times hess_L[k] (dense: per
        component), or solved against cov_L[k]^T when only the dense cov_L[k] is known.  Returns the views of that buffer.
        """
        tr = self._traj
        for k in tr.lay.keys:
            x = self.x[k]
            m = self.pdist[k]() if self.pdist is not None else torch.randn(x.numel(), device=x.device, dtype=x.dtype)
            if self.diag_mass[k]:
                m, L = m.reshape(x.shape), self.hess_L[k]
                tr.pv[k].copy_(m if L is None else L * m)
                continue
            m = m.to(x.dtype).reshape(-1)
            cols = torch.view_as_real(m) if m.is_complex() else m[:, None]           # one column per component
            if self.hess_L[k] is not None:
                cols = self.hess_L[k] @ cols
            else:
                cols = torch.linalg.solve_triangular(self.cov_L[k].T, cols, upper=True)
            m = torch.view_as_complex(cols.contiguous()) if x.is_complex() else cols[:, 0]
            tr.pv[k].copy_(m.reshape(x.shape))
        return tr.pv


class HMC(_DenseMass, sampler.HMC):
    """
    sampler.HMC with a dense mass per key: the constructor of sampler.HMC, with diag_mass a bool or a dict by key and, for a key
    with diag_mass[k] false, cov_L[k] (and optionally hess_L[k]) the real (n, n) lower-triangular Cholesky factor of the covariance
    (of the mass matrix), as a tensor, an hmat.DenseMat or an hmat.TriangMat.  A move of Nstep steps is 2 (Nstep + 2) launches.
    """


class NUTS(_DenseMass, nuts.NUTS):
    """
    nuts.NUTS with a dense mass per key (see HMC): a leaf is four launches and one readback, the move's starting energy two.
    """
    _kinetic_launches = 2

    def _leaf(self, edge, direction, H_start, far):
        lay, tr = self._lay, self._traj
        eps, h = self._step_args(direction)
        table, new_buf = self._blocks.table(), lambda: torch.empty(lay.N, dtype=lay.rdtype, device=lay.device)
        q1, p_half, p1, g1 = new_buf(), new_buf(), new_buf(), lay.new()
        project(table, edge.p, edge.g, eps, self._c, 0.5 * h, p_half, tr.z)
        drift(table, tr.z, edge.q, eps, self._c, h, q1)
        with torch.enable_grad():
            grad = self.dUdx(lay.views(q1))
        lay.pack(grad, g1)
        project(table, p_half, g1, eps, self._c, 0.5 * h, p1, tr.z)
        if far is None:
            drift(table, tr.z, None, None, self._c, 0.0, None, out=self._out, ws=tr.ws)
        else:
            drift(table, tr.z, q1, None, self._c, 0.0, None, p=p1, q_far=far.q, p_far=far.p, out=self._out, ws=tr.ws)
        self.launches += 4
        new = nuts._State(lay, q1, p1, g1)
        K, a_far, a_near = self._out.tolist()                                # the one readback of a leaf
        if far is not None:
            new.minus_angle, new.plus_angle = (a_far, a_near) if direction > 0 else (-a_near, -a_far)
        U_new = self._U
        H_new = K + self._logdetM + float(U_new)
        states = [(new.qv, new.pv, U_new)] if self.track_states else None
        return nuts.TreeInfo(new, new, new, U_new, H_new, nuts._logaddexp(-H_start, -H_new), False,
                             bool(self.is_divergent(H_start, H_new)), states)
