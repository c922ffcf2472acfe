"""
The No-U-Turn sampler on the two tree-leaf kernels of csrc/nuts.hip: the counterpart of the reference's sampler.NUTS and TreeInfo
(sampler.py:922-1335; Hoffman & Gelman 2014, with the progressive sampling of Betancourt 2017, A.3.2) for the masses sampler.HMC
takes.  sampler.NUTS and sampler.TreeInfo stay the refusing stubs they were; the sampler lives here.

A leaf of the tree is one leapfrog step from an edge of the tree built so far, and it is exactly
  1. rime_nuts_leaf_open: the half kick and the drift from the edge state (read only) into freshly allocated flat q and p,
  2. one evaluation of the potential on the views of that q,
  3. one pack of its gradient into a fresh flat g,
  4. rime_nuts_leaf_close: the second half kick in place, and in the same pass the kinetic energy and the two projections
     (q - q_far) . p_far and (q - q_far) . p of the no-U-turn criterion against the far edge of the move's base tree (its left
     edge when the direction is +1, its right edge when it is -1),
  5. one readback of those three doubles.
No clone, no torch reduction, no deepcopy: a closed leaf state is never written again, and trees share leaf states by
reference, so a merge moves references.  The within-subtree criteria the reference computes and then overwrites are not
computed; the criterion that survives every merge inside build_tree is the one between the base tree's far edge and the merged
tree's outer edge, which is what the outer leaf's close returned.  Every energy and weight is a Python float, every decision a
comparison of floats, and the np.random draws come in the reference's order (one rand per doubling for the direction if
sample_direction, one per merge in recursion order, the Metropolis rand; randint only on a restart), so a seeded chain makes the
reference's decisions.  `launches` counts kernel launches (two per leaf and one energy-only pass per move), `fn_evals` the
potential evaluations (one per leaf and one per move).  There is no CPU path.

Not provided:
  * DynamicStepSize / StepSize: the reference's end-of-step eps.update(prob) has no counterpart while sampler.StepSize and
    sampler.DynamicStepSize refuse
  * RecycledHMC
  * Betancourt's generalised (momentum-sum) no-U-turn criterion, which the reference names as a TODO: the criterion is
    Hoffman & Gelman's
and what sampler.HMC refuses is refused here in the same words: dense and hmat mass matrices, pmask, complex step sizes.
Dense mass matrices per key are massmat.NUTS, which replaces the leaf by the launches of csrc/massmat.hip.
"""
import math

import numpy as np
import torch

from . import _lib, sampler
from .ops import _stream, _ptr
from .paramdict import ParamDict


def leaf_open(q0, p0, g0, q1, p1, eps, c, h):
    """
    One launch of rime_nuts_leaf_open on flat real vectors (see include/rime_hip.h): q0, p0, g0 read only; q1, p1 written;
    eps, c may be None; h the signed step.
    """
    N, code = sampler._check_vectors('nuts', 'leaf_open', p0, (q0, g0, q1, p1, eps, c))
    with torch.cuda.device(p0.device):
        _lib.check(_lib.lib.rime_nuts_leaf_open(code, N, _ptr(q0), _ptr(p0), _ptr(g0), _ptr(q1), _ptr(p1), _ptr(eps), _ptr(c),
                                                float(h), _stream()), 'rime_nuts_leaf_open')


def leaf_close(q1, p1, g1, eps, c, h, q_far, p_far, out, ws=None):
    """
    One launch of rime_nuts_leaf_close on flat real vectors (see include/rime_hip.h): p1 in place; q1, g1, q_far, p_far read
    only (q_far and p_far both None: no projections); out a float64 tensor of three elements on the device; ws the workspace
    (allocated if None or short).
    """
    N, code = sampler._check_vectors('nuts', 'leaf_close', p1, (q1, g1, eps, c, q_far, p_far))
    sampler._check_out('nuts', out, p1.device)
    ws = sampler._workspace(_lib.lib.rime_nuts_workspace(N), p1.device, ws)
    with torch.cuda.device(p1.device):
        _lib.check(_lib.lib.rime_nuts_leaf_close(code, N, _ptr(q1), _ptr(p1), _ptr(g1), _ptr(eps), _ptr(c), float(h), _ptr(q_far),
                                                 _ptr(p_far), _ptr(out), _ptr(ws), ws.numel() * 8, _stream()),
                   'rime_nuts_leaf_close')


def _logaddexp(x, y):
    lo, hi = (x, y) if x < y else (y, x)
    return math.log1p(math.exp(lo - hi)) + hi


class _State:
    """one phase-space point of a tree: flat q, p and gradient, and their views; never written once its leaf is closed"""
    __slots__ = ('q', 'p', 'g', 'qv', 'pv', 'gv', 'minus_angle', 'plus_angle')

    def __init__(self, lay, q, p, g, gv=None):
        self.q, self.p, self.g = q, p, g
        self.qv, self.pv = lay.views(q), lay.views(p)
        self.gv = lay.views(g) if gv is None else gv
        self.minus_angle = self.plus_angle = None         # Hoffman & Gelman's two projections against the base tree's far edge


class TreeInfo:
    """
    A (sub)tree of one NUTS move: the reference's thirteen fields and `states`.  The edges and the proposal are leaf states
    shared by reference (left, right, prop); q_left, p_left, grad_left, q_right, p_right, grad_right, q_prop and p_prop are the
    ParamDict views of their flat buffers.  q_prop_U and q_prop_H are the proposal's potential and Hamiltonian, weight the log
    of the tree's summed weights, turning and diverging its flags, states the list of (q, p, U) from left to right or None.
    """
    def __init__(self, left, right, prop, q_prop_U, q_prop_H, weight, turning=False, diverging=False, states=None):
        self.left, self.right, self.prop = left, right, prop
        self.q_prop_U, self.q_prop_H, self.weight = q_prop_U, q_prop_H, weight
        self.turning, self.diverging, self.states = turning, diverging, states

    q_left = property(lambda self: self.left.qv)
    p_left = property(lambda self: self.left.pv)
    grad_left = property(lambda self: self.left.gv)
    q_right = property(lambda self: self.right.qv)
    p_right = property(lambda self: self.right.pv)
    grad_right = property(lambda self: self.right.gv)
    q_prop = property(lambda self: self.prop.qv)
    p_prop = property(lambda self: self.prop.pv)


class NUTS(sampler.HMC):
    """
    No-U-Turn sampler (reference sampler.NUTS): sampler.HMC with a trajectory that doubles until it turns, diverges or reaches
    max_tree_depth.  The arguments are the reference's: those of sampler.HMC without Nstep and U0, and
    max_tree_depth : most doublings of a move;  biased : biased progressive sampling between trees (False: uniform);
    track_states : keep (q, p, U) of every state of a move's tree in TreeInfo.states;  sample_direction : draw the direction of
    every doubling (False: always forward).  After a move that ends in its Metropolis test `_base_tree` is its tree.
    """
    _kinetic_launches = 1                                    # launches of the move's starting energy (massmat.NUTS: two)

    def __init__(self, potential_fn, x0, eps, cov_L=None, hess_L=None, diag_mass=True, pdist=None, pmask=None, dHmax=1000,
                 record_divergences=False, max_tree_depth=6, biased=True, track_states=False, sample_direction=True):
        super().__init__(potential_fn, x0, eps, cov_L=cov_L, hess_L=hess_L, diag_mass=diag_mass, Nstep=1, pdist=pdist, pmask=pmask,
                         dHmax=dHmax, record_divergences=record_divergences)
        self.max_tree_depth = max_tree_depth
        self.biased = biased
        self.track_states = track_states
        self.sample_direction = sample_direction
        self.launches = 0
        self._out = torch.zeros(3, dtype=torch.float64, device=self._lay.device)
        self._ws = sampler._workspace(_lib.lib.rime_nuts_workspace(self._lay.N), self._lay.device)

    # ------------------------------------------------------------------ the criterion and the merge
    def is_turning(self, tree):
        """Hoffman & Gelman's criterion between the two edges of a tree (two dot products in plain torch)"""
        return sampler.hoffman_uturn(tree.q_left, tree.q_right, tree.p_left, tree.p_right)

    def merge_trees(self, old_tree, new_tree, new_tree_right):
        """
        The two trees as one, by (biased) progressive sampling: one np.random.rand() decides whose proposal lives on; the outer
        edge is the new tree's (the right one if new_tree_right), the inner edge the old tree's.  The inputs are not modified.
        """
        if self.biased:
            d = new_tree.weight - old_tree.weight
        else:
            d = new_tree.weight - _logaddexp(old_tree.weight, new_tree.weight)
        new_prob = 1.0 if d >= 0 else math.exp(d)
        keep = new_tree if np.random.rand() < new_prob else old_tree
        left, right = (old_tree, new_tree) if new_tree_right else (new_tree, old_tree)
        states = None if keep.states is None else left.states + right.states
        return TreeInfo(left.left, right.right, keep.prop, keep.q_prop_U, keep.q_prop_H, _logaddexp(old_tree.weight, new_tree.weight),
                        old_tree.turning or new_tree.turning, old_tree.diverging or new_tree.diverging, states)

    # ------------------------------------------------------------------ the tree
    def _step_args(self, direction):
        """(eps vector or None, signed launch scalar) of a leaf in this direction"""
        if isinstance(self._eps_flat, torch.Tensor):
            return self._eps_flat, float(direction)
        return None, float(direction) * self._eps_flat

    def _leaf(self, edge, direction, H_start, far):
        """the depth-0 tree one step from `edge`, with its projections against the state `far` (None: not computed)"""
        lay = self._lay
        eps, h = self._step_args(direction)
        q1 = torch.empty(lay.N, dtype=lay.rdtype, device=lay.device)
        p1 = torch.empty(lay.N, dtype=lay.rdtype, device=lay.device)
        leaf_open(edge.q, edge.p, edge.g, q1, p1, eps, self._c, h)
        new = _State(lay, q1, p1, lay.new())
        with torch.enable_grad():
            grad = self.dUdx(new.qv)
        lay.pack(grad, new.g)
        leaf_close(q1, p1, new.g, eps, self._c, h, None if far is None else far.q, None if far is None else far.p, self._out, self._ws)
        self.launches += 2
        K, a_far, a_near = self._out.tolist()                                # the one readback of a leaf
        if far is not None:                                                   # (q+ - q-) . p-  and  (q+ - q-) . p+
            new.minus_angle, new.plus_angle = (a_far, a_near) if direction > 0 else (-a_near, -a_far)
        U_new = self._U
        H_new = K + self._logdetM + float(U_new)
        states = [(new.qv, new.pv, U_new)] if self.track_states else None
        return TreeInfo(new, new, new, U_new, H_new, _logaddexp(-H_start, -H_new), False, bool(self.is_divergent(H_start, H_new)), states)

    def _as_state(self, q, p, dUdq0):
        if isinstance(q, _State):
            return q
        lay = self._lay
        if dUdq0 is None:
            with torch.enable_grad():
                dUdq0 = self.dUdx(q)
        return _State(lay, lay.pack(q, lay.new()), lay.pack(p, lay.new()), lay.pack(dUdq0, lay.new()))

    @torch.no_grad()
    def build_tree(self, q, p, direction, tree_depth, H_start, dUdq0=None, base_tree=None):
        """
        The subtree of 2^tree_depth leaves that continues from the state (q, p) in `direction` (+1 or -1): q, p ParamDicts with
        dUdq0 the gradient at q if known, or q a state of a tree (an edge of a TreeInfo: tree.left, tree.right) and p, dUdq0
        unused.  base_tree: the tree the subtree will be merged into; its far edge is what every merged subtree is tested
        against (None: the subtree's own two edges).  Always built in full; returns a TreeInfo.
        """
        edge = self._as_state(q, p, dUdq0)
        far = None if base_tree is None else (base_tree.left if direction > 0 else base_tree.right)
        return self._build(edge, direction, tree_depth, float(H_start), far)

    def _build(self, edge, direction, depth, H_start, far):
        if depth == 0:
            return self._leaf(edge, direction, H_start, far)
        half_tree = self._build(edge, direction, depth - 1, H_start, far)
        other_tree = self._build(half_tree.right if direction > 0 else half_tree.left, direction, depth - 1, H_start, far)
        merged = self.merge_trees(half_tree, other_tree, new_tree_right=direction > 0)
        if far is None:
            turning = self.is_turning(merged)
        else:
            outer = merged.right if direction > 0 else merged.left
            turning = (outer.minus_angle < 0) or (outer.plus_angle < 0)
        merged.turning = merged.turning or turning
        return merged

    # ------------------------------------------------------------------ the move
    @torch.no_grad()
    def step(self, sample_p=True):
        """
        One NUTS move with its Metropolis decision; sample_p=False starts from the stored momentum self.p instead of a fresh
        draw.  Returns (accept, prob) as 0-d tensors.
        """
        tr, lay = self._traj, self._lay
        if sample_p:
            self.draw_momentum()
        else:
            lay.pack(self.p, tr.p)
        K_start = tr.kinetic(self._c) + self._logdetM
        self.launches += self._kinetic_launches
        q0 = lay.pack(self.x, lay.new())
        start = _State(lay, q0, tr.p.clone(), lay.new())
        with torch.enable_grad():
            dUdq0 = self.dUdx(start.qv)
        lay.pack(dUdq0, start.g)
        U_start = self._U
        H_start = K_start + float(U_start)

        states = [(start.qv, start.pv, U_start)] if self.track_states else None
        base_tree = TreeInfo(start, start, start, U_start, H_start, -H_start, False, False, states)
        tree_depth = 0
        new_tree, direction = None, 1.0
        while tree_depth < self.max_tree_depth:
            direction = (1.0 if np.random.rand() > 0.5 else -1.0) if self.sample_direction else 1.0
            edge = base_tree.right if direction > 0 else base_tree.left
            far = base_tree.left if direction > 0 else base_tree.right
            new_tree = self._build(edge, direction, tree_depth, H_start, far)
            if new_tree.diverging or new_tree.turning:
                break
            base_tree = self.merge_trees(base_tree, new_tree, direction > 0)
            tree_depth += 1
        self._last = dict(K_start=K_start, H_start=H_start, H_end=base_tree.q_prop_H, tree_depth=tree_depth)
        is_potential = isinstance(self.potential_fn, sampler.Potential)

        if new_tree is not None and new_tree.diverging:
            Nchain = len(self.Uchain)
            if self.record_divergences:
                outer = new_tree.right if direction > 0 else new_tree.left
                self._divergences.append((Nchain, outer.qv, outer.pv))
            if Nchain > 0 and tree_depth < 2:                       # close to the origin: restart from a random entry of the chain
                i = np.random.randint(0, Nchain)
                self._U, self._gradU = self.Uchain[i], None
                self.x = ParamDict({k: torch.as_tensor(self.chain[k][i], device=self.x[k].device) for k in self.x})
                if is_potential:
                    self.potential_fn.prob.update(self.x)
                return torch.tensor(False), torch.tensor(0.0, dtype=torch.float64)

        # Python's min, as the reference's: a NaN exponential leaves 1
        prob = min(1.0, math.exp(min(H_start - base_tree.q_prop_H, 700.0)))
        accept = bool(np.random.rand() < prob)
        self._base_tree = base_tree
        if accept:
            self.x = base_tree.q_prop.clone()
            self.p = base_tree.p_prop.clone()
            self._U, self._gradU = base_tree.q_prop_U, None
        else:
            self._U, self._gradU = U_start, dUdq0
        if is_potential:                                            # the model stands at the last leaf: put it where the chain is
            self.potential_fn.prob.update(self.x)
        return torch.tensor(accept), torch.tensor(prob, dtype=torch.float64)
