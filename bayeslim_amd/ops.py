"""
torch.autograd.Function wrappers over the C-ABI of librime_hip.so (include/rime_hip.h).

These are the only callers of the native library.  Every function requires CUDA (ROCm)
tensors and raises otherwise -- there is no CPU path in the product.

  fringe_sum   : vis = sum_pix psky * exp(+-2 pi i nu/c b.s)     rime_model.py:423-429 +
                                                                 telescope_model.py:310-358
  interp_gather: out[..., p] = sum_k w[p,k] m[..., inds[p,k]]    utils.py:815-861
  alm2pix      : out = Re(alm @ Ylm)                             sph_harm.py:1342-1372
"""
import contextlib
import ctypes
import os
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, RIME_F32, RIME_F64

TILE = 64        # pixel-axis padding granule required by the fringe kernels (rime::TP)

# bench.py sets this to a list to collect (kernel name, start event, end event, fringe elements)
# around every fringe-sum launch; None (default) records nothing.
PROFILE = None


def _require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("bayeslim_amd ops need tensors on the GPU (got device '%s'); "
                               "there is no CPU implementation" % t.device)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _cptr(t):
    """a complex tensor as the (re, im) pairs the library reads; None: the null pointer"""
    return _ptr(torch.view_as_real(t) if t is not None else None)


def _dtype_code(dtype):
    if dtype in (torch.float32, torch.complex64):
        return RIME_F32
    if dtype in (torch.float64, torch.complex128):
        return RIME_F64
    raise TypeError('unsupported dtype %s' % dtype)


def _real_dtype(t):
    code = _dtype_code(t.dtype)
    return code, (torch.float32 if code == RIME_F32 else torch.float64)


def _dense(t, dtype=None):
    """t detached, its conjugation resolved, in `dtype` (None: its own) and contiguous: an operand read through one pointer"""
    t = t.detach().resolve_conj()
    return (t if dtype is None else t.to(dtype)).contiguous()


def _host_array(x, flat=False, integer=None):
    """x (a tensor on any device, an array or a sequence) as a numpy array on the host; flat: as one axis; integer: the
    ValueError message for a non-empty array of another kind (an empty sequence arrives as float64 and passes)"""
    a = np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)
    if flat:
        a = a.reshape(-1)
    if integer is not None and a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(integer)
    return a


def _workspace(nbytes, device, floor=0):
    """(buffer, its size) for a rime_*_workspace() answer.  floor=16: the callers whose kernels always get a pointer; floor=0:
    those that pass the null pointer with zero bytes (_ptr(None)).  Which one a call takes is part of its C contract."""
    n = max(int(nbytes), floor)
    return (torch.empty(n, dtype=torch.uint8, device=device) if n else None), n


def _timed(name, *fields):
    """context that appends (name, start event, end event) + fields + what the body puts into the list it is given to
    PROFILE, read once on entry.  PROFILE None: no event, the body is given None.  A body that raises records nothing."""
    prof = PROFILE
    return _NOT_TIMED if prof is None else _record(prof, name, fields)


_NOT_TIMED = contextlib.nullcontext()


@contextlib.contextmanager
def _record(prof, name, fields):
    e0, e1, late = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), []
    e0.record()
    yield late
    e1.record()
    prof.append((name, e0, e1) + fields + tuple(late))


class _IndexPlan:
    """
    Base of the plans built with numpy on the host: the attributes named in `_TABLES` as int32 tensors, made on first use per
    device, kept in self.__dict__['_tabs'] (LMPlan keeps its keyed tables there too) and dropped on pickling and copies.
    """
    _TABLES = ()

    def _cache(self):
        return self.__dict__.setdefault('_tabs', {})

    def tables(self, device):
        """dict of the int32 tables on `device`, cached"""
        key, tabs = str(torch.device(device)), self._cache()
        if key not in tabs:
            tabs[key] = {k: torch.as_tensor(getattr(self, k), dtype=torch.int32, device=device).contiguous() for k in self._TABLES}
        return tabs[key]

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_tabs', None)
        return state


def pad_to_tile(n):
    return ((int(n) + TILE - 1) // TILE) * TILE


class FringeGeometry:
    """
    Everything the fringe kernels need besides psky: baseline vectors, per-time pointing
    vectors, frequencies and the baseline -> beam-model-pair grouping.  Built once per RIME
    minibatch and reused by forward and backward.

    blvecs (Nbl, 3) [m]; sdir (Nt, 3, Pstride) unit vectors, zero-padded past each time's
    pixel count; freqs (Nf,) [Hz]; bl_mp: optional beam-model-pair index per baseline (Nmp pairs,
    mp_pairs = their (model1, model2) tuples: needed for the matrix-core path with several models);
    antpos (Nant, 3) + bl_ants (antenna-index pairs) enable the antenna-factored matrix-core kernels;
    group: antennas per block group of that path (default 128; 32 / 64 for rank-local tile shards).
    """
    def __init__(self, blvecs, sdir, freqs, bl_mp=None, Nmp=1, conj=False, npix=None,
                 antpos=None, bl_ants=None, mfma='auto', ant_like=None, mp_pairs=None, group=None):
        _require_cuda(blvecs, sdir)
        dev = blvecs.device
        self.blvecs = blvecs.detach().to(torch.float64).contiguous()
        self.sdir = sdir.detach().to(torch.float64).contiguous()
        f = torch.as_tensor(freqs, dtype=torch.float64)
        fh = f.detach().cpu().numpy()
        self.freqs = f.to(dev).contiguous()
        self.Nbl, self.Nt, self.Nf = self.blvecs.shape[0], self.sdir.shape[0], len(fh)
        self.Pstride = self.sdir.shape[2]
        assert self.sdir.shape[1] == 3 and self.Pstride % TILE == 0
        self.sign = -1 if conj else 1
        # algorithmic fringe elements per launch: Nbl x Nf x (valid pixels summed over times)
        nvalid = int(sum(npix)) if npix is not None else self.Nt * self.Pstride
        self.elements = self.Nbl * self.Nf * nvalid
        self.max_blen = float(torch.linalg.norm(self.blvecs, dim=1).max().item())
        # channel grid: 1 = exactly uniform (rotation recurrence), 2 = uniform up to tiny residuals
        # (float32-rounded linspace: recurrence + first-order correction), 0 = arbitrary
        # nu_phi: the largest phase residual [rad] the near-uniform kernels correct to first order only (they drop
        # phi^2 / 2: fine for float32 below 2e-3, for float64 only below NU_F64_PHI -- see _fringe_call)
        self.f0 = float(fh[0])
        self.nu_phi = 0.0
        if len(fh) > 1:
            self.df = float((fh[-1] - fh[0]) / (len(fh) - 1))
            eps = np.abs(fh - (self.f0 + self.df * np.arange(len(fh)))).max()
            phi = 2 * np.pi * eps * max(self.max_blen, 1.0) / 2.99792458e8
            if eps <= 1e-9 * max(abs(self.df), 1.0):
                self.uniform = 1
            elif phi < 2e-3 and self.df != 0:
                self.uniform = 2
                self.nu_phi = float(phi)
            else:
                self.uniform = 0
        else:
            self.uniform, self.df = 1, 0.0
        # antenna factorisation (matrix-core path): baselines given as antenna-index pairs
        self.ant = None
        if mfma is not False and ant_like is not None and ant_like.ant is not None and ant_like.Nbl == self.Nbl:
            # same baseline set as an existing geometry (another time minibatch): share its pair tables
            per16 = self.Nt * self.Nf * (self.Pstride // 16) * 32768
            self.ant = dict(ant_like.ant, mfma_flops_fwd=per16 * ant_like.ant['mfma_fwd'],
                            mfma_flops_bwd=per16 * ant_like.ant['mfma_bwd'])
            if self.Nt > 65535:
                self.ant = None
        elif antpos is not None and bl_ants is not None and mfma in ('auto', True):
            self._setup_antenna_path(antpos, bl_ants, force=(mfma is True), bl_mp=bl_mp if int(Nmp) > 1 else None,
                                     mp_pairs=mp_pairs, group=group or MFMA_GROUP)
        # model-pair grouping
        self.Nmp = int(Nmp)
        if bl_mp is None or self.Nmp == 1:
            self.Nmp = 1
            self.mp_offsets = (ctypes.c_int * 2)(0, self.Nbl)
            self.bl_order = None
        else:
            bl_mp = np.asarray(bl_mp, dtype=np.int64)
            order = np.argsort(bl_mp, kind='stable')
            counts = np.bincount(bl_mp, minlength=self.Nmp)
            offs = np.concatenate([[0], np.cumsum(counts)])
            self.mp_offsets = (ctypes.c_int * (self.Nmp + 1))(*[int(o) for o in offs])
            self.bl_order = torch.as_tensor(order, dtype=torch.int32, device=dev)

    def _setup_antenna_path(self, antpos, bl_ants, force=False, bl_mp=None, mp_pairs=None, group=None):
        """enable the antenna-factored matrix-core kernels when the baseline set suits them: self.ant"""
        group = group or MFMA_GROUP
        Nant = int(antpos.shape[0])
        bl_ants = [(int(a), int(b)) for a, b in bl_ants]
        ant_model = _antenna_models(self, Nant, bl_ants, force, bl_mp, mp_pairs)
        if ant_model is False:
            return
        posh = antpos.detach().to(torch.float64).cpu().numpy()
        # a point-symmetric array of more than 128 antennas with one beam model: symmetric groups (_pair_cross_plan)
        plan = None
        if PAIR_CROSS and MIRROR and PAIR and ant_model is None and group == MFMA_GROUP and Nant > MFMA_GROUP:
            plan = _pair_cross_plan(posh, bl_ants)
        raw = _antenna_blocks(bl_ants, Nant, bl_mp if ant_model is not None else None, ant_model, group,
                              groups=None if plan is None else plan['ants'])
        if raw is None:
            return
        # the factorisation must reproduce the baseline vectors it replaces
        dev = self.blvecs.device
        pos = antpos.detach().to(torch.float64).to(dev).contiguous()
        i1 = torch.as_tensor([a for a, _ in bl_ants], device=dev)
        i2 = torch.as_tensor([b for _, b in bl_ants], device=dev)
        if not torch.allclose(pos[i2] - pos[i1], self.blvecs, rtol=0, atol=1e-9):
            return
        blocks = [_plain_block(r, pos, dev) for r in raw]
        ant = dict(blocks=blocks, Nant=Nant, two_pass_mask=_two_pass_mask(blocks, raw, self.Nbl, dev), multi_model=ant_model is not None)
        if MIRROR:
            ant.update(_symmetric_forms(blocks, raw, posh, plan, dev, self.Nbl))
        # executed matrix-core work per real-psky pass, from the blocks that run it: MFMAs per 16 pixels (_mfma_counts) of
        # 2*32*32*16 flop each
        run = ant.get('blocks_real', blocks)
        per16 = self.Nt * self.Nf * (self.Pstride // 16) * 32768
        ant['mfma_fwd'], ant['mfma_bwd'] = sum(b['mf_fwd'] for b in run), sum(b['mf_bwd_real'] for b in run)
        ant['mfma_flops_fwd'], ant['mfma_flops_bwd'] = per16 * ant['mfma_fwd'], per16 * ant['mfma_bwd']
        self.ant = ant


def _env_int(name, default):
    """C atoi() of an environment variable (leading integer, else 0), as csrc/ reads its switches"""
    v = os.environ.get(name)
    if v is None:
        return default
    import re
    m = re.match(r'\s*([+-]?\d+)', v)
    return int(m.group(1)) if m else 0


# float64 calls take the near-uniform kernels (MODE_ROT_NU: first-order channel correction, phi^2 / 2 dropped) only while
# that term stays inside the float64 contract of 1e-11: phi < 1e-6 drops at most 5e-13 per fringe value; beyond it they
# take the MODE_DIRECT kernels (one sincos per channel).  float32 keeps the 2e-3 bound of FringeGeometry (2e-6 dropped).
NU_F64_PHI = 1e-6

MFMA_MIN_ANTS = int(os.environ.get('RIME_MFMA_MIN_ANTS', '16'))   # 'auto' threshold (see _setup_antenna_path)
MFMA_GROUP = 128          # antennas per group of the matrix-core path (4 x 4 tiles of 32)
MFMA_MAX_ANTS = 2048      # table memory only: 136 blocks x 128 KB at 2048 antennas
# complex psky, forward: diagonal blocks whose baselines all have one orientation run as
# triangular self-cross blocks in ONE pass (RIME_SELF_BLOCKS=0: the two real-plane passes of the diagonal kernel)
SELF_BLOCKS = os.environ.get('RIME_SELF_BLOCKS', '1') != '0'
# arrays of 33..48 antennas: the forward kernel with the second row tile's re / im planes packed into one operand
# (csrc/fringe_mfma.hip, fringe_ant_fwd_packed_kernel); RIME_FWD_PACKED=0 keeps the generic two-tile kernel (A/B)
FWD_PACKED = _env_int('RIME_FWD_PACKED', 1) != 0         # parsed as the library parses it (atoi)


def _group_capacity(n, group):
    """rows a group of n antennas occupies in a cross block: 32, 64 or 128 (the kernels' shapes)"""
    if group <= 32 or n <= 32:
        return 32
    return 64 if (group <= 64 or n <= 64) else 128


def _antenna_blocks(bl_ants, Nant, bl_mp=None, ant_model=None, group=MFMA_GROUP, groups=None):
    """
    Block decomposition of the pair matrix for the matrix-core path (see include/rime_hip.h).
    Antennas are ordered by (beam model, index) and cut into groups of <= `group` antennas that share
    a beam model; every (group pair, beam-model pair) that holds a baseline becomes one block with its
    own psky plane `mp`:
      diagonal block: one group against itself (upper-triangular 32 x 32 tiles),
      cross block   : group I x group J, rows padded to a supported shape (32, 32), (32, 64), (64, 64)
                      or (128, 128) antenna rows.
    Returns a list of dicts {ants_i, ants_j | None, rows_i, rows_j, mp, direct, conj, cpass}, tables
    int32 [128, 128] of baseline slots indexed by LOCAL antenna indices, or None when a pair occurs
    twice (not representable).  cpass: +1 the block holds direct entries only, -1 conj entries only,
    0 both (a complex psky then takes one pass per real plane).
    groups: the antenna groups themselves (lists of antenna indices, each of <= MFMA_GROUP, together every antenna once)
    in place of the cut by index -- the symmetric groups of _pair_cross_plan.  Every block carries the indices gi, gj of its groups.
    """
    if ant_model is None:
        ant_model = [0] * Nant
    gid, lid = {}, {}
    if groups is None:
        order = sorted(range(Nant), key=lambda a: (ant_model[a], a))
        groups = []
        for a in order:
            if not groups or ant_model[groups[-1][0]] != ant_model[a] or len(groups[-1]) >= group:
                groups.append([])
            gid[a], lid[a] = len(groups) - 1, len(groups[-1])
            groups[-1].append(a)
    else:
        groups = [list(g) for g in groups]
        for g, ants in enumerate(groups):
            for k, a in enumerate(ants):
                gid[a], lid[a] = g, k
        assert len(gid) == Nant == sum(len(g) for g in groups) and max(len(g) for g in groups) <= MFMA_GROUP
    tabs = {}

    def get(key):
        if key not in tabs:
            tabs[key] = (_slot_table(), _slot_table())
        return tabs[key]

    for b, (a1, a2) in enumerate(bl_ants):
        mp = 0 if bl_mp is None else int(bl_mp[b])
        g1, l1, g2, l2 = gid[a1], lid[a1], gid[a2], lid[a2]
        if g1 == g2:
            direct, conj = get((g1, g1, mp))
            if l1 // 32 <= l2 // 32:
                tab, i, j = direct, l1, l2
            else:
                tab, i, j = conj, l2, l1
        elif g1 < g2:
            tab, i, j = get((g1, g2, mp))[0], l1, l2           # baseline I_i -> J_j: V[i, j]
        else:
            tab, i, j = get((g2, g1, mp))[1], l2, l1           # baseline J_j -> I_i: conj(V[i, j])
        if tab[i, j] >= 0:
            return None
        tab[i, j] = b
    blocks = []

    def compact(tab, rows, cols):
        out = _slot_table()
        out[:len(rows), :len(cols)] = tab[np.ix_(rows, cols)]
        return out

    for (gi, gj, mp) in sorted(tabs):
        direct, conj = tabs[(gi, gj, mp)]
        nd, nc = int((direct >= 0).sum()), int((conj >= 0).sum())
        # antennas of the groups that hold no baseline of this block are dropped (a rank-local shard of a
        # block, a sparse pair set): fewer generated rows, possibly a smaller kernel shape
        used = (direct >= 0) | (conj >= 0)
        if gi == gj:
            keep = np.nonzero(used.any(0) | used.any(1))[0]
            # tile membership (index // 32) decides direct vs conj inside a diagonal block: only drop whole
            # trailing / unused 32-antenna tiles' worth when the order of the rest is unchanged
            if len(keep) < len(groups[gi]) and np.array_equal(keep // 32, np.arange(len(keep)) // 32):
                direct, conj = compact(direct, keep, keep), compact(conj, keep, keep)
                ants_i = [groups[gi][k] for k in keep]
            else:
                ants_i = groups[gi]
            blk = dict(ants_i=ants_i, ants_j=None, rows_i=len(ants_i), rows_j=0, mp=mp, gi=gi, gj=gj,
                       cpass=(1 if nc == 0 else (-1 if nd == 0 else 0)))
        else:
            ri, cj_ = np.nonzero(used.any(1))[0], np.nonzero(used.any(0))[0]
            direct, conj = compact(direct, ri, cj_), compact(conj, ri, cj_)
            blk = dict(ants_i=[groups[gi][k] for k in ri], ants_j=None, rows_i=len(ri), rows_j=0, mp=mp, gi=gi, gj=gj,
                       cpass=(1 if nc == 0 else (-1 if nd == 0 else 0)))
            gi_ants, gj_ants = blk['ants_i'], [groups[gj][k] for k in cj_]
        if gi != gj:
            ci, cj = _group_capacity(len(gi_ants), group), _group_capacity(len(gj_ants), group)
            if (ci, cj) not in ((32, 32), (32, 64), (64, 32), (64, 64), (128, 128)):
                ci = cj = 128                                # unequal groups: padded to the full shape
            ai, aj = gi_ants, gj_ants
            if ci > cj:
                # the kernels take the smaller group as I: swap the groups (V[j, i] = conj(V[i, j]))
                ai, aj, ci, cj = aj, ai, cj, ci
                direct, conj = conj.T.copy(), direct.T.copy()
                blk['cpass'] = -blk['cpass']
            blk.update(ants_i=ai, ants_j=aj, rows_i=ci, rows_j=cj)
        blk['direct'], blk['conj'] = direct, conj
        blocks.append(blk)
    return blocks


# MIRROR PAIRS (round 5; csrc/fringe_mfma.hip, "MIRROR PAIRS"): antennas with r' - c = -(r - c) have conjugate phasors.
MIRROR = _env_int('RIME_MIRROR', 1) != 0        # RIME_MIRROR=0: no search (every row evaluated, rounds 1-4)
MIRROR_TOL = 1e-9                               # [m] mismatch allowed in r + r' = 2 c (7e-10 turn of phase at 200 MHz)


def _mirror_pairs(P, tol=MIRROR_TOL):
    """
    Point symmetry of a set of antenna positions P (n, 3): the centre c shared by the largest number of pairs
    (r_a + r_b = 2 c within `tol`, all three coordinates) and a maximal pairing about it.  Returns (c, pairs, singles) --
    pairs of row indices (a, b), singles the rows without a partner (an antenna AT the centre is its own mirror: a single) --
    or None when fewer than two pairs exist.  O(n^2) on the host, n <= 128 per block.
    """
    P = np.asarray(P, dtype=np.float64)
    n = len(P)
    if n < 4:
        return None
    ia, ib = np.triu_indices(n, 1)
    sums = P[ia] + P[ib]
    # vote for 2 c on a 1-micrometre grid (a symmetric set of m antennas puts ~m / 2 of its n (n - 1) / 2 pair sums in one cell;
    # twice, with the grid shifted by half a cell, so that sums sitting on a cell edge are not split)
    best = None
    for shift in (0.0, 0.5):
        q = np.floor(sums * 1e6 + shift).astype(np.int64)
        cells, inv, cnt = np.unique(q, axis=0, return_inverse=True, return_counts=True)
        k = int(np.argmax(cnt))
        if best is None or cnt[k] > best[0]:
            best = (int(cnt[k]), sums[np.asarray(inv).reshape(-1) == k].mean(axis=0))
    if best[0] < 2:
        return None
    c2 = best[1]
    D = np.abs(P[:, None, :] + P[None, :, :] - c2).max(-1) <= tol
    partner = -np.ones(n, dtype=np.int64)
    for a in range(n):
        if partner[a] >= 0:
            continue
        for b in np.nonzero(D[a])[0]:
            if b != a and partner[b] < 0:
                partner[a], partner[b] = b, a
                break
    pairs = [(a, int(partner[a])) for a in range(n) if partner[a] > a]
    singles = [a for a in range(n) if partner[a] < 0]
    if len(pairs) < 2:
        return None
    # the centre the pairs actually share (mean of their sums: the kernels use E' = conj(E) EXACTLY for a pair)
    c = np.mean([P[a] + P[b] for a, b in pairs], axis=0) / 2
    if max(np.abs(P[a] + P[b] - 2 * c).max() for a, b in pairs) > tol:
        return None
    return c, pairs, singles


def _mirror_order(P, packed=None):
    """
    Row order of a diagonal block that puts mirror pairs into the octet pairs of 16-row groups: rows 16 g + i (i < 8) and
    16 g + 8 + i of the groups g < Gm hold the two antennas of a pair (or a single and an empty row); the other antennas
    fill plain groups behind them.  Returns (rows, mask, centre): rows[r] = index into P or -1 (empty row), mask = bit per
    mirror group -- or None when no order with at least one mirror group fits into the block's row capacity
    32 ceil(n / 32) (the kernel shape of the plain order must not grow).  `packed`: 33..48 antennas on the packed forward
    kernel -- 48 rows, mirror groups in the first row tile only.
    """
    found = _mirror_pairs(P)
    if found is None:
        return None
    c, pairs, singles = found
    n = len(P)
    packed = (32 < n <= 48 and FWD_PACKED) if packed is None else packed
    G = 3 if packed else (32 * ((n + 31) // 32)) // 16              # 16-row groups available
    Gcap = 2 if packed else G                                       # groups that may be mirror groups
    for Gm in range(min(Gcap, (len(pairs) + 7) // 8), 0, -1):
        slots = 8 * Gm
        pin = min(len(pairs), slots)
        sin = min(len(singles), slots - pin)
        if n - 2 * pin - sin <= 16 * (G - Gm):
            break
    else:
        return None
    rows = [-1] * (16 * G)
    for k, (a, b) in enumerate(pairs[:pin]):
        rows[16 * (k // 8) + k % 8], rows[16 * (k // 8) + 8 + k % 8] = a, b
    for k, a in enumerate(singles[:sin], start=pin):
        rows[16 * (k // 8) + k % 8] = a                             # its mirror row stays empty
    rest = [x for ab in pairs[pin:] for x in ab] + list(singles[sin:])
    rows[16 * Gm:16 * Gm + len(rest)] = rest
    while rows and rows[-1] < 0:
        rows.pop()
    return rows, (1 << Gm) - 1, c


# THE BLOCK PLAN.  A block is a dict; the mirror, pair and pair cross forms below are their plain block on new rows.


def _mfma_counts(kind, ri, rj=0, hub=False):
    """(mf_fwd, mf_bwd, mf_bwd_real, mf_self) of one block: MFMAs per 16-pixel K step of the real-psky forward, the one-pass
    complex backward, the real-psky backward and the one-pass complex forward (None: the form has no such pass).  A full
    32 x 32 antenna tile takes 12 MFMAs of 2*32*32*16 flop (3 hi/lo products x 4 real products)."""
    if kind == 'diag':
        # ri antennas in TA row tiles: 12 per tile above the diagonal; a diagonal tile 7 forward (symmetric products folded) and
        # 9 backward (symmetric form, round 3); 33..48 antennas on the packed forward: 7 + 6 + 3 = 16 (round 4); the complex
        # passes run all TA (TA + 1) / 2 tiles in full (mf_self: where the block runs as a self block, _plain_block)
        TA = (ri + 31) // 32
        off, full = 12 * (TA * (TA - 1) // 2), 12 * (TA * (TA + 1) // 2)
        return 16 if (32 < ri <= 48 and FWD_PACKED) else off + 7 * TA, full, off + 9 * TA, full
    if kind == 'cross':                                      # ri x rj rows of the kernel's shape: every tile in full
        mf = 12 * (ri // 32) * (rj // 32)
        return mf, mf, mf, None
    if kind == 'pair':
        # ri rows: one row tile (<= 32 rows, no hub) 7 and 9 as a diagonal tile; two row tiles 26 (against 63 / 100 of the
        # three- / four-tile plain kernels) and 30
        return 26 if ri > 32 or hub else 7, None, 30 if ri > 32 else 9, None
    # forward 12 on each of the four tiles whatever the row counts (48); backward 12 per (row tile of I that holds a row, 16 rows
    # of J that hold a row) and 32 pixels (64 x 64 rows: 48).  A mirror block keeps the counts of its plain block.
    assert kind == 'xpair', kind
    return 48, None, 6 * ((ri + 31) // 32) * ((rj + 15) // 16), None


def _slot_table(rows=MFMA_GROUP):
    return np.full((rows, MFMA_GROUP), -1, dtype=np.int32)


def _assert_slots_once(slots, *tables):
    """every baseline slot of `slots` sits in exactly one entry of `tables` (a row order must never drop or double one)"""
    out = np.sort(np.concatenate([t[t >= 0] for t in tables]))
    assert np.array_equal(out, np.sort(slots)) and (np.diff(out) > 0).all()


def _remap_tables(od, oc, vrow, hub=None):
    """
    The slot tables of a diagonal block on new rows, numpy in and out.  od[i, j] = b: baseline b runs from antenna i to antenna
    j, oc[i, j] = b: from j to i (_antenna_blocks); vrow[a]: the row of antenna a.  Returns (direct, conj, centre): a baseline
    from row r1 to row r2 sits in direct[r1, r2] where r1's row tile is not behind r2's, else in conj[r2, r1]; the baselines of
    `hub`, an antenna served outside the rows, in centre[0, r] (hub -> row r) or centre[1, r] (row r -> hub) (None: no hub).
    None when the hub's autocorrelation is asked for (not a column sum of the image).
    """
    od, oc = (np.asarray(t).reshape(MFMA_GROUP, MFMA_GROUP) for t in (od, oc))
    (i, j), (k, l) = np.nonzero(od >= 0), np.nonzero(oc >= 0)
    a1, a2 = np.concatenate([i, l]), np.concatenate([j, k])            # every baseline runs from antenna a1 to antenna a2
    slot = np.concatenate([od[i, j], oc[k, l]])
    h1, h2 = a1 == (-1 if hub is None else hub), a2 == (-1 if hub is None else hub)
    if (h1 & h2).any():
        return None
    r1, r2 = np.asarray(vrow)[a1], np.asarray(vrow)[a2]
    assert (r1[~h1] >= 0).all() and (r2[~h2] >= 0).all()                # every antenna has a row
    direct, conj, centre = _slot_table(), _slot_table(), (None if hub is None else _slot_table(2))
    if hub is not None:
        centre[0, r2[h1]] = slot[h1]
        centre[1, r1[h2]] = slot[h2]
    up = ~(h1 | h2) & (r1 // 32 <= r2 // 32)
    down = ~(h1 | h2) & (r1 // 32 > r2 // 32)
    direct[r1[up], r2[up]] = slot[up]
    conj[r2[down], r1[down]] = slot[down]
    _assert_slots_once(slot, *(t for t in (direct, conj, centre) if t is not None))
    return direct, conj, centre


def _derived_block(blk, dev, pos, direct, conj, mf=None, **keys):
    """the plain block `blk` on new rows: their positions and slot tables on `dev`, the counts `mf` the form has of its own
    (_mfma_counts), the keys of the form; one real plane per call (no single complex pass forward, no self block)"""
    dev_t = lambda x: torch.as_tensor(x, device=dev).contiguous()
    keys.update({k: v for k, v in zip(('mf_fwd', 'mf_bwd', 'mf_bwd_real'), mf or ()) if v is not None})
    return dict(blk, pos=dev_t(pos), direct=dev_t(direct.reshape(-1)), conj=dev_t(conj.reshape(-1)), fwd_cpass=0,
                self_pos=None, mf_self=0, **keys)


def _plain_tables(blk, host):
    """(direct, conj) of the plain block `blk` as numpy: `host`, the arrays its device tables were made from, where the caller
    still has them, else read back from the device"""
    return host if host is not None else tuple(blk[k].cpu().numpy() for k in ('direct', 'conj'))


def _mirror_block(blk, P, dev, host=None):
    """the mirrored form of a built diagonal block (see _mirror_order): positions measured from the centre of symmetry in
    the new row order, pair tables rebuilt for it, `mirror` mask; None when the block has no usable symmetry"""
    n = int(blk['nrows'])
    if blk['cross'] != 0 or n < 4:
        return None
    found = _mirror_order(P)
    if found is None:
        return None
    rows, mask, c = found
    newrow = -np.ones(n, dtype=np.int64)
    pos = np.zeros((len(rows), 3))
    for r, a in enumerate(rows):
        if a >= 0:
            newrow[a], pos[r] = r, P[a] - c
    assert (newrow >= 0).all() and len(rows) <= 32 * ((n + 31) // 32)
    direct, conj, _ = _remap_tables(*_plain_tables(blk, host), newrow)
    nd, nc = int((direct >= 0).sum()), int((conj >= 0).sum())
    return _derived_block(blk, dev, pos, direct, conj, nrows=len(rows), mirror=int(mask), rows=list(rows),
                          cpass=(1 if nc == 0 else (-1 if nd == 0 else 0)))


# CONJUGATE-PAIR FORM (round 5; csrc/fringe_mfma.hip, "CONJUGATE-PAIR FORM"): a diagonal block of a point-symmetric array
# contracted from the phasors of one antenna of every mirror pair.
PAIR = _env_int('RIME_PAIR', 1) != 0            # RIME_PAIR=0: such blocks keep the mirror-pair kernels (A/B measurements)
PAIR_ROWS = 64                                  # rows of the pair kernels (firsts + antennas without a partner)
PAIR_CPLX = _env_int('RIME_PAIR_CPLX', 1) != 0  # complex psky on pair blocks, one pass per real plane (0: the plain blocks; A/B)
# round 6: rows ordered so that octets hold two 4-term progressions of one step; the pair backward kernel rotates within them
# (0: the plain row order here AND no rotation in the library, which reads the same variable -- round 5's result bit for bit)
PAIR_AP = _env_int('RIME_PAIR_AP', 1) != 0


def _pair_layout(P, rows=PAIR_ROWS, hub_ok=True, ap=False):
    """
    Rows of the conjugate-pair form for antenna positions P (n, 3): (firsts, partner, hub, centre) -- firsts[k] the antenna
    of row k, partner[k] its mirror antenna or -1, hub the antenna AT the centre that is served outside the rows (or None)
    -- or None when the set has no point symmetry or does not fit: at most `rows` rows, plus (hub_ok) the hub when the rows
    are full.  ap: the same rows in the order of the pair BACKWARD (_pair_ap_order); the forward keeps the plain order, and
    with it every bit of its result.
    """
    found = _mirror_pairs(P)
    if found is None:
        return None
    c, pairs, singles = found
    hub = None
    if len(pairs) + len(singles) > rows:
        at_c = [a for a in singles if np.abs(np.asarray(P[a]) - c).max() <= MIRROR_TOL]
        if not hub_ok or not at_c or len(pairs) + len(singles) - 1 > rows:
            return None
        hub = at_c[0]
        singles = [a for a in singles if a != hub]
    firsts = [a for a, _ in pairs] + list(singles)
    partner = [b for _, b in pairs] + [-1] * len(singles)
    if ap:
        order = _pair_ap_order(np.asarray(P, dtype=np.float64)[firsts] - c)
        firsts, partner = [firsts[k] for k in order], [partner[k] for k in order]
    return firsts, partner, hub, c


def _pair_ap_mask(pos):
    """
    The octet mask the pair backward kernel derives from its row positions `pos` (nrows, 3) (csrc/fringe_mfma.hip,
    fringe_pair_bwd_kernel: the same test, restated): with the block's step d = pos[1] - pos[0], bit m is set when rows
    8m..8m+3 and 8m+4..8m+7 both are r, r + d, r + 2d, r + 3d within MIRROR_TOL in every coordinate.
    """
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    if n < 8:
        return 0
    d = pos[1] - pos[0]
    mask = 0
    for m in range(n // 8):
        ok = all(np.abs(pos[q + k] - pos[q] - k * d).max() <= MIRROR_TOL for q in (8 * m, 8 * m + 4) for k in (1, 2, 3))
        mask |= int(ok) << m
    return mask


def _pair_ap_order(pos):
    """
    Row order of the conjugate-pair form that exposes arithmetic progressions to the pair backward kernel, which evaluates
    one phasor of a quad r, r + d, r + 2d, r + 3d and rotates it to the other three: a permutation of
    range(len(pos)) whose leading octets hold two such quads each, all with ONE step d; every other row follows in its old
    order.  d is the candidate among the array's shortest separations that yields the most quads (the first such
    candidate in row order).  The representative of a mirror pair is NOT swapped: the rows are the rows of the plain order,
    so every phasor keeps its phase and the forward computes what it computed.  The identity when fewer than two quads
    exist -- arrays without lattice lines keep their order.
    """
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    ident = list(range(n))
    if n < 8:
        return ident
    diff = pos[None, :, :] - pos[:, None, :]                       # diff[a, b] = pos[b] - pos[a]
    length = np.sqrt((diff ** 2).sum(-1))
    length[np.arange(n), np.arange(n)] = np.inf
    short = length.min()
    if not np.isfinite(short) or short <= MIRROR_TOL:
        return ident
    cands = []                                                      # steps of the shortest length, one of +d / -d each
    for a, b in zip(*np.nonzero(length <= short * (1 + 1e-6))):
        d = diff[a, b]
        if not any(np.abs(d - e).max() <= MIRROR_TOL or np.abs(d + e).max() <= MIRROR_TOL for e in cands):
            cands.append(d)
    best = []
    for d in cands:
        succ = -np.ones(n, dtype=np.int64)                          # succ[a]: the row at pos[a] + d
        for a in range(n):
            hit = np.nonzero(np.abs(diff[a] - d).max(-1) <= MIRROR_TOL)[0]
            if len(hit):
                succ[a] = hit[0]
        has_pred = set(succ[succ >= 0].tolist())
        quads = []
        for a in range(n):
            if a in has_pred:
                continue
            line = [a]
            while succ[line[-1]] >= 0 and succ[line[-1]] not in line:
                line.append(int(succ[line[-1]]))
            quads += [line[4 * q:4 * q + 4] for q in range(len(line) // 4)]
        if quads:
            # what the kernel will test: offsets from the quad's first row against multiples of the step of the FIRST quad
            step = pos[quads[0][1]] - pos[quads[0][0]]
            quads = [q for q in quads if all(np.abs(pos[q[k]] - pos[q[0]] - k * step).max() <= MIRROR_TOL for k in (1, 2, 3))]
        if len(quads) > len(best):
            best = quads
    noct = len(best) // 2
    if noct == 0:
        return ident
    lead = [a for q in best[:2 * noct] for a in q]
    taken = set(lead)
    order = lead + [a for a in ident if a not in taken]
    assert sorted(order) == ident
    return order


def _pair_rows(firsts, partner):
    """{antenna: virtual row} of the pair forms: row k holds firsts[k], row 64 + k its mirror antenna"""
    rows = {int(a): k for k, a in enumerate(firsts)}
    rows.update({int(b): 64 + k for k, b in enumerate(partner) if b >= 0})
    return rows


def _rows_from_centre(P, rows, c):
    """(pos, flat): the positions of the antennas `rows` measured from the centre c.  A coplanar array measured from a centre
    in its plane has z = 0 within the tolerance of the pairing itself -> exactly 0 and the `flat` licence (the kernels skip that
    term of the phase)"""
    pos = np.asarray(P)[rows] - c
    flat = int(np.abs(pos[:, 2]).max() <= MIRROR_TOL)
    if flat:
        pos[:, 2] = 0.0
    return pos, flat


def _pair_block(blk, P, dev, host=None):
    """the conjugate-pair form of a built diagonal block (include/rime_hip.h, rime_fringe_pair_fwd_block): positions of the
    rows from the centre of symmetry, the pair tables of the virtual 128-row block (row k: firsts[k], row 64 + k: its
    mirror), the hub's slot table; None when the block does not qualify.  More than 64 antennas: up to 64 rows + the hub (two
    row tiles); 33..64 antennas: up to 32 rows (one row tile); up to 32 antennas keep the one-tile kernels (the same MFMAs,
    _mfma_counts; their generation is already halved by the mirror pairs)."""
    n = int(blk['nrows'])
    if blk['cross'] != 0 or n <= 32:
        return None
    lay = _pair_layout(P) if n > 64 else _pair_layout(P, rows=32, hub_ok=False)
    if lay is None:
        return None
    firsts, partner, hub, c = lay
    od, oc = _plain_tables(blk, host)

    def tables(firsts, partner):
        vrow = -np.ones(n, dtype=np.int64)
        rows = _pair_rows(firsts, partner)
        vrow[list(rows)] = list(rows.values())
        return _remap_tables(od, oc, vrow, hub)

    tabs = tables(firsts, partner)
    if tabs is None:
        return None                                          # the hub's autocorrelation is asked for
    direct, conj, centre = tabs
    pos, flat = _rows_from_centre(P, firsts, c)
    dev_t = lambda x: torch.as_tensor(x, device=dev).contiguous()
    # the backward's own row order (round 6, _pair_ap_order): the same rows permuted, tables rebuilt for them; the forward keeps
    # the plain order, so no bit of it moves
    bwd = None
    order = _pair_ap_order(pos) if PAIR_AP else list(range(len(firsts)))
    if order != list(range(len(firsts))):
        bf, bp = [firsts[k] for k in order], [partner[k] for k in order]
        bd, bc, bcen = tables(bf, bp)
        bwd = dict(firsts=bf, partner=bp, pos=dev_t(pos[order]), direct=dev_t(bd.reshape(-1)), conj=dev_t(bc.reshape(-1)),
                   centre=None if hub is None else dev_t(bcen.reshape(-1)))
    return _derived_block(blk, dev, pos, direct, conj, _mfma_counts('pair', len(firsts), hub=hub is not None), nrows=len(firsts),
                          mirror=0, pair=1, firsts=list(firsts), partner=list(partner), hub=hub, flat=flat, bwd=bwd, cpass=0,
                          centre=None if hub is None else dev_t(centre.reshape(-1)))


# PAIR CROSS BLOCKS (csrc/fringe_xpair.hip): a point-symmetric array of MORE than MFMA_GROUP antennas.  The cut by index makes
# groups that are not symmetric sets; here the ROWS of the conjugate-pair form (firsts, then antennas without a partner) are cut
# into groups of <= PAIR_ROWS, a group being its rows together with their mirror antennas -- symmetric about the one centre c.
# Diagonal blocks: the pair form above, unchanged.  The block between two groups: four real products of their rows' images.
PAIR_CROSS = _env_int('RIME_PAIR_CROSS', 1) != 0       # RIME_PAIR_CROSS=0: the groups by index and the generic cross blocks


def _plain_plan_cost(P, bl_ants, group=MFMA_GROUP):
    """(MFMAs per 16-pixel K step, generated rows) of the real-psky forward on the groups cut by index, for the baselines
    asked for: a diagonal block on the conjugate-pair form where its group is a symmetric set that fits (an estimate on the
    host: the hub's autocorrelation and unused antennas are not looked at), a cross block only between groups that share a
    baseline"""
    P = np.asarray(P, dtype=np.float64)
    Nant = len(P)
    sizes = [min(group, Nant - k) for k in range(0, Nant, group)]
    mf = rows = 0
    for g, n in enumerate(sizes):
        lay = None
        if n > 32 and PAIR:
            lay = _pair_layout(P[g * group:g * group + n]) if n > 64 else _pair_layout(P[g * group:g * group + n], rows=32, hub_ok=False)
        if lay is not None:
            mf += _mfma_counts('pair', len(lay[0]), hub=lay[2] is not None)[0]
            rows += len(lay[0])
        else:
            mf += _mfma_counts('diag', n)[0]
            rows += n
    shared = {(min(a // group, b // group), max(a // group, b // group)) for a, b in bl_ants if a // group != b // group}
    for x, y in shared:
        ci, cj = _group_capacity(sizes[x], group), _group_capacity(sizes[y], group)
        if (ci, cj) not in ((32, 32), (32, 64), (64, 32), (64, 64), (128, 128)):
            ci = cj = 128
        mf += _mfma_counts('cross', ci, cj)[0]
        rows += sizes[x] + sizes[y]
    return mf, rows


def _pair_cross_plan(antpos, bl_ants, rows=PAIR_ROWS):
    """
    Plan of a point-symmetric array with more than MFMA_GROUP antennas, on the host from numpy inputs alone: antpos (Nant, 3),
    bl_ants the antenna pairs of the baselines in slot order.  Returns None when the array does not qualify (no symmetry of
    the whole set, a pair listed twice, so many antennas without a partner that the plan contracts or generates no less than
    the groups by index), else a dict
      centre  c (3,)
      groups  [dict(firsts, partner)]: antenna of every row and its mirror antenna (-1: none), <= `rows` rows each, sizes balanced
              (no tail group too small for the pair form of its diagonal block)
      ants    [firsts + partners of each group]: the groups for _antenna_blocks
      cross   {(gi, gj), gi < gj: dict(rows_i, rows_j, pos (rows_i + rows_j, 3) from c, flat, direct, conj)} for the group pairs that
              share a baseline; direct / conj int32 [128, 128] by virtual row (k: row k of I, 64 + k: its mirror) and virtual
              column (the same for J): direct[r, c] = slot of the baseline r -> c, conj[r, c] = slot of c -> r.
    """
    P = np.asarray(antpos, dtype=np.float64)
    Nant = len(P)
    if Nant <= MFMA_GROUP or Nant > MFMA_MAX_ANTS or P.ndim != 2 or P.shape[1] != 3:
        return None
    found = _mirror_pairs(P)
    if found is None:
        return None
    c, pairs, singles = found
    firsts = [a for a, _ in pairs] + list(singles)
    partner = [b for _, b in pairs] + [-1] * len(singles)
    R = len(firsts)
    G = (R + rows - 1) // rows
    if G < 2:
        return None                                       # (more than 128 antennas in <= 64 rows cannot be)
    size = (R + G - 1) // G
    groups = [dict(firsts=firsts[k:k + size], partner=partner[k:k + size]) for k in range(0, R, size)]
    assert len(groups) == G and all(len(g['firsts']) <= rows for g in groups)
    gid, vrow = {}, {}
    for g, grp in enumerate(groups):
        grp_rows = _pair_rows(grp['firsts'], grp['partner'])
        vrow.update(grp_rows)
        gid.update(dict.fromkeys(grp_rows, g))
    assert len(gid) == Nant
    # the tables of a cross block are filled from the baseline list itself (no plain block exists yet), rows from group I and
    # columns from group J, the orientation decided by the order of the GROUPS -- not by row tiles as inside a diagonal block
    # (_remap_tables); what the two share: the virtual rows and the exactly-once check
    cross, slots = {}, {}
    seen = set()
    for slot, (a1, a2) in enumerate(bl_ants):
        a1, a2 = int(a1), int(a2)
        if (a1, a2) in seen:
            return None
        seen.add((a1, a2))
        g1, g2 = gid[a1], gid[a2]
        if g1 == g2:
            continue
        key = (min(g1, g2), max(g1, g2))
        if key not in cross:
            cross[key], slots[key] = dict(direct=_slot_table(), conj=_slot_table()), []
        slots[key].append(slot)
        if g1 < g2:
            cross[key]['direct'][vrow[a1], vrow[a2]] = slot          # I -> J: V[r, c]
        else:
            cross[key]['conj'][vrow[a2], vrow[a1]] = slot            # J -> I: conj(V[r, c])
    # cost against the groups by index: matrix work and generated rows, both must shrink; every group costed as a pair block of
    # two row tiles (64 rows), whatever its rows
    bl = [(int(a), int(b)) for a, b in bl_ants]
    mf_new = _mfma_counts('pair', 64)[0] * G + _mfma_counts('xpair', 64, 64)[0] * len(cross)
    rows_new = R + sum(len(groups[gi]['firsts']) + len(groups[gj]['firsts']) for gi, gj in cross)
    mf_old, rows_old = _plain_plan_cost(P, bl)
    if mf_new >= mf_old or rows_new >= rows_old:
        return None
    for (gi, gj), blk in cross.items():
        _assert_slots_once(slots[gi, gj], blk['direct'], blk['conj'])
        fi, fj = groups[gi]['firsts'], groups[gj]['firsts']
        pos, flat = _rows_from_centre(P, fi + fj, c)
        blk.update(rows_i=len(fi), rows_j=len(fj), pos=pos, flat=flat)
    return dict(centre=c, groups=groups, cross=cross,
                ants=[g['firsts'] + [b for b in g['partner'] if b >= 0] for g in groups])


def _pair_cross_block(blk, plan_blk, dev):
    """the device form of one block of _pair_cross_plan in place of the built plain cross block `blk` (include/rime_hip.h,
    rime_fringe_pair_cross_fwd_block)"""
    ri, rj = int(plan_blk['rows_i']), int(plan_blk['rows_j'])
    return _derived_block(blk, dev, plan_blk['pos'], plan_blk['direct'], plan_blk['conj'], _mfma_counts('xpair', ri, rj),
                          nrows=ri + rj, rows_i=ri, rows_j=rj, xpair=1, mirror=0, flat=int(plan_blk['flat']), cpass=0)


def _dense_strides(t):
    """element strides (time, model pair, pol product, channel) of a (Nt,Nmp,Npp,Nf,P) tensor whose
    pixel axis is contiguous, or None when the tensor cannot be passed as is"""
    if t.stride(-1) != 1:
        return None
    st = t.stride()
    P = t.shape[-1]
    if t.shape[3] > 1 and st[3] < P:
        return None
    if any(s <= 0 and n > 1 for s, n in zip(st[:4], t.shape[:4])):
        return None
    return (ctypes.c_longlong * 4)(*[int(max(s, 1)) for s in st[:4]])


def _pow2_scale(amax):
    """power of two s with amax * s in [2^13, 2^14]; 1 where amax == 0 (exact to apply and undo)"""
    safe = torch.where(amax > 0, amax, torch.ones_like(amax))
    e = torch.floor(torch.log2(16384.0 / safe)).clamp(-100.0, 100.0)      # denormal-sized rows: no inf scale
    return torch.where(amax > 0, torch.exp2(e), torch.ones_like(amax))


def _block_launch(blk, backward, cflag):
    """
    how one planned block is launched: (entry point, its leading arguments, its slot tables, the complex-pass flag where the
    entry point takes one, MFMAs per 16 pixels).  Kinds: self (forward only: a diagonal block in one complex pass, as the
    cross block of its rows with themselves), xpair and pair (one real plane per call), plain (cflag != 0: one complex pass).
    """
    d = 'bwd' if backward else 'fwd'
    rows, flag, mf = blk, (), blk['mf_bwd_real'] if backward else blk['mf_fwd']
    if not backward and cflag != 0 and blk['cross'] == 0:
        n = int(blk['self_pos'].shape[0])
        name, lead, flag, mf = 'rime_fringe_ant_fwd_block', (_ptr(blk['self_pos']), n, n, 0), (cflag,), blk['mf_self']
    elif blk.get('xpair'):
        name, lead = 'rime_fringe_pair_cross_%s_block' % d, (_ptr(blk['pos']), blk['rows_i'], blk['rows_j'], blk['flat'])
    elif blk.get('pair'):
        if backward:
            rows = blk.get('bwd') or blk                         # the backward's own row order, where one exists
        name, lead = 'rime_fringe_pair_%s_block' % d, (_ptr(rows['pos']), blk['nrows'], _ptr(rows['centre']), blk['flat'])
    else:
        name, lead, flag = 'rime_fringe_ant_%s_block' % d, (_ptr(blk['pos']), blk['nrows'], blk['cross'], blk['mirror']), (cflag,)
        if backward and cflag != 0:
            mf = blk['mf_bwd']
    return name, lead, (_ptr(rows['direct']), _ptr(rows['conj'])), flag, mf


def _fringe_ant_call(geom, backward, inp, out, strides, Npp, cplx):
    """
    antenna-factored kernels: one launch per block of the pair matrix (ops._antenna_blocks), each on
    the psky plane of its beam-model pair.  Real psky: one pass per polarisation product.  Complex
    psky (V is linear in psky: V[ar + i ai] = V[ar] + i V[ai]; d/d(ai) = Re(conj(F) (-i g))): blocks
    whose entries all have one orientation take ONE complex pass (forward: cross blocks; backward:
    every block, the imaginary plane is a second lane-local contraction of the same products); the
    others take one pass per real plane.  Returns the MFMA flops executed.
    """
    a = geom.ant
    # real psky: mirror / pair forms where the array has them; complex psky: the plain blocks (single-pass forms where a
    # block's baselines allow), except where a block has the conjugate-pair form -- V is linear in psky, so that block takes
    # one pair pass per real plane (2 x 26 MFMAs per K step against 120 of the one-pass self block of 128 antennas)
    blocks = a.get('blocks_cplx', a['blocks']) if cplx else a.get('blocks_real', a['blocks'])
    tp_mask = a.get('two_pass_mask_cplx', a['two_pass_mask']) if cplx else a['two_pass_mask']
    m = 2 if cplx else 1                                     # floats per psky element
    st_t, st_mp, st_pp, st_f = (int(strides[k]) * m for k in range(4))
    Nbl, Nt, Nf, Nmp = geom.Nbl, geom.Nt, geom.Nf, geom.Nmp
    dev = inp.device
    geo = (_ptr(geom.sdir), _ptr(geom.freqs))
    shape = (Nbl, Nt, Nf, geom.Pstride, st_t, st_f, m, geom.sign)
    per16 = Nt * Nf * (geom.Pstride // 16) * 32768
    flops = 0
    if not backward:
        # inp: psky (Nt, Nmp, Npp, Nf, Ps[, 2]) float32 view; out: vis (Npp, Nbl, Nt, Nf, 2) float32
        if cplx and inp.stride(-1) == 1 and inp.stride(-2) == 2 and all(inp.stride(k) % 2 == 0 for k in range(4)):
            # interleaved complex rows: scale from max(|re|, |im|) and the minimum of each plane in ONE pass (round 4; torch's
            # abs + amax + amin passes were 1.1 ms of a C5 rank step)
            scale = torch.empty((Nmp, Npp, Nt, Nf), dtype=torch.float32, device=dev)
            rowmin = [torch.empty_like(scale), torch.empty_like(scale)]
            check(lib.rime_fringe_row_scale_cplx(_ptr(inp), Nmp, Npp, Nt, Nf, inp.stride(1) // 2, inp.stride(2) // 2,
                                                 inp.stride(0) // 2, inp.stride(3) // 2, inp.shape[-2], _ptr(scale),
                                                 _ptr(rowmin[0]), _ptr(rowmin[1]), _stream()), 'rime_fringe_row_scale_cplx')
        elif cplx:
            amax = inp.abs().amax(dim=(-1, -2))                                    # (Nt, Nmp, Npp, Nf)
            lo = inp.amin(dim=-2)                                                  # (Nt, Nmp, Npp, Nf, 2): per plane
            rowmin = [lo[..., c].permute(1, 2, 0, 3).contiguous() for c in range(2)]
            scale = _pow2_scale(amax.permute(1, 2, 0, 3)).contiguous()             # (Nmp, Npp, Nt, Nf)
        elif inp.stride(-1) == 1:
            # one launch: power-of-two scale and minimum of every (mp, pp, t, f) row, through the view's strides
            scale = torch.empty((Nmp, Npp, Nt, Nf), dtype=torch.float32, device=dev)
            rowmin = [torch.empty_like(scale)]
            check(lib.rime_fringe_row_scale(_ptr(inp), Nmp, Npp, Nt, Nf, inp.stride(1), inp.stride(2), inp.stride(0),
                                            inp.stride(3), inp.shape[-1], _ptr(scale), _ptr(rowmin[0]), _stream()),
                  'rime_fringe_row_scale')
        else:
            lo, hi = torch.aminmax(inp, dim=-1)                                    # one pass, no |psky| temporary
            amax = torch.maximum(hi, -lo)
            rowmin = [lo.permute(1, 2, 0, 3).contiguous()]
            scale = _pow2_scale(amax.permute(1, 2, 0, 3)).contiguous()             # (Nmp, Npp, Nt, Nf)
        ws, _ = _workspace(lib.rime_fringe_ant_workspace(Nbl, Nt, Nf, geom.Pstride), dev, 16)
        two_pass = [blk for blk in blocks if cplx and blk['fwd_cpass'] == 0]
        tmp = torch.empty((Nbl, Nt, Nf, 2), dtype=torch.float32, device=dev) if two_pass else None

        def launch(blk, pp, c, cflag):
            mp = blk['mp']
            src = ctypes.c_void_p(inp.data_ptr() + 4 * (mp * st_mp + pp * st_pp + c))     # pair forms: c picks the real plane
            name, lead, tables, flag, mf = _block_launch(blk, False, cflag)
            check(getattr(lib, name)(*lead, *geo, src, _ptr(scale[mp, pp]), _ptr(rowmin[c][mp, pp]), *tables, *shape, *flag,
                                     _ptr(ws), ws.numel(), _stream()), name)
            return mf

        for pp in range(Npp):
            for blk in blocks:
                single = cplx and blk['fwd_cpass'] != 0
                flops += launch(blk, pp, 0, blk['fwd_cpass'] if single else 0)
            check(lib.rime_fringe_ant_fwd_finish(_ptr(ws), ws.numel(), _ptr(out[pp]), Nbl, Nt, Nf, geom.Pstride,
                                                 _stream()), 'rime_fringe_ant_fwd_finish')
            if two_pass:                                     # V += i V[ai] on the baselines of those blocks
                for blk in two_pass:
                    flops += launch(blk, pp, 1, 0)
                check(lib.rime_fringe_ant_fwd_finish(_ptr(ws), ws.numel(), _ptr(tmp), Nbl, Nt, Nf, geom.Pstride,
                                                     _stream()), 'rime_fringe_ant_fwd_finish')
                if len(two_pass) < len(blocks):
                    tmp *= tp_mask                           # slots of single-pass blocks hold stale values
                out[pp][..., 0] -= tmp[..., 1]
                out[pp][..., 1] += tmp[..., 0]
    else:
        # inp: gvis as real (Npp, Nbl, Nt, Nf, 2); out: gpsky float32 view with psky's strides
        ws, _ = _workspace(lib.rime_fringe_ant_bwd_workspace(Nbl, Nt, Nf), dev, 16)
        gvt = ws[:Nt * Nf * 2 * Nbl * 4].view(torch.float32).view(Nt * Nf, 2 * Nbl)    # what bwd_prepare writes
        two_pass = [blk for blk in blocks if cplx and blk['cpass'] == 0]
        for pp in range(Npp):
            written = set()
            for c in range(2 if two_pass else 1):
                g = inp[pp] if c == 0 else torch.stack([inp[pp][..., 1], -inp[pp][..., 0]], dim=-1).contiguous()
                check(lib.rime_fringe_ant_bwd_prepare(_ptr(g), Nbl, Nt, Nf, _ptr(ws), ws.numel(), _stream()),
                      'rime_fringe_ant_bwd_prepare')
                if c == 0:
                    # max |gvis| per (t, f) from the transposed copy: a contiguous row reduction (the same
                    # reduction over the (Nbl, Nt, Nf, 2) layout is strided and 4x slower); -i g has the same maxima
                    scale_pp = torch.empty(Nt * Nf, dtype=torch.float32, device=dev)
                    check(lib.rime_fringe_row_scale(_ptr(gvt), 1, 1, 1, Nt * Nf, 0, 0, 0, 2 * Nbl, 2 * Nbl, _ptr(scale_pp),
                                                    None, _stream()), 'rime_fringe_row_scale')
                # single-pass blocks first: they initialise BOTH planes of their psky slice, the two-pass
                # blocks then accumulate plane by plane
                todo = sorted(blocks, key=lambda b: not (cplx and b['cpass'] != 0)) if c == 0 else two_pass
                for blk in todo:
                    single = cplx and blk['cpass'] != 0
                    mp = blk['mp']
                    planes = [(mp, 0), (mp, 1)] if single else [(mp, c)]
                    acc = int(planes[0] in written)
                    assert all((pl in written) == bool(acc) for pl in planes)
                    written.update(planes)
                    dst = ctypes.c_void_p(out.data_ptr() + 4 * (mp * st_mp + pp * st_pp + (0 if single else c)))
                    name, lead, tables, flag, mf = _block_launch(blk, True, blk['cpass'] if single else 0)
                    check(getattr(lib, name)(*lead, *geo, _ptr(scale_pp), *tables, *shape, *flag, acc, dst,
                                             _ptr(ws), ws.numel(), _stream()), name)
                    flops += mf
            assert len(written) == Nmp * m, 'every psky plane must be written by a block'
    return flops * per16


def _antenna_models(geom, Nant, bl_ants, force, bl_mp, mp_pairs):
    """whether the baseline set suits the antenna-factored kernels, and the beam model of every antenna: False (it does not),
    None (one model for all) or the list of models"""
    if Nant > MFMA_MAX_ANTS or len(bl_ants) != geom.Nbl or geom.Nt > 65535:      # (reduce kernels: t on grid.z)
        return False
    # worth it when the array needs at least two 32-antenna tiles and most pairs are requested
    # (measured against the baseline-formulation kernels: 128 antennas / 8128 baselines 4.8x (fwd)
    # and 5.8x (bwd) faster; 37 antennas / 666 baselines 1.1x and 1.6x faster; 19 antennas 1.7x and
    # 1.1x slower)
    if not force and (Nant < MFMA_MIN_ANTS or geom.Nbl < Nant * Nant // 8):
        return False
    # several beam models: every antenna must carry ONE model (beam_model.py:303-327 pairs models per baseline)
    if bl_mp is not None and mp_pairs is not None and len(mp_pairs) > 1:
        ant_model = [None] * Nant
        for (a1, a2), mp in zip(bl_ants, bl_mp):
            for ant, mdl in ((a1, mp_pairs[mp][0]), (a2, mp_pairs[mp][1])):
                if ant_model[ant] is None:
                    ant_model[ant] = mdl
                elif ant_model[ant] != mdl:
                    return False
        return [0 if mdl is None else mdl for mdl in ant_model]
    if bl_mp is not None and any(int(x) != 0 for x in bl_mp):            # (bl_mp is only passed when Nmp > 1)
        # without a model table the blocks read psky plane 0: several planes, or one plane that is not plane 0,
        # stay on the baseline-formulation kernels
        return False
    return None


def _plain_block(r, pos, dev):
    """the block `r` of _antenna_blocks as the kernels take it: the positions of its rows (pos: every antenna, on `dev`), its
    tables on `dev`, its counts"""
    pi = pos[torch.as_tensor(r['ants_i'], device=dev)]
    self_pos, mf_self = None, 0
    if r['ants_j'] is None:
        rows, (mf_fwd, mf_bwd, mf_bwd_real, mf_full) = pi.contiguous(), _mfma_counts('diag', pi.shape[0])
        cross, fwd_cpass = 0, 0                              # forward diagonal blocks: one real plane per call ...
        if SELF_BLOCKS and r['cpass'] != 0:
            # ... unless psky is complex and every baseline has one orientation: then the block runs as the
            # triangular cross block of the group with itself, ONE complex pass (rime_fringe_ant_fwd_block
            # with cross == Nrows)
            self_pos = torch.zeros((pi.shape[0] + 31) // 32 * 32, 3, dtype=torch.float64, device=dev)
            self_pos[:pi.shape[0]] = pi
            fwd_cpass, mf_self = r['cpass'], mf_full
    else:
        pj = pos[torch.as_tensor(r['ants_j'], device=dev)]
        rows = torch.zeros(r['rows_i'] + r['rows_j'], 3, dtype=torch.float64, device=dev)
        rows[:pi.shape[0]] = pi
        rows[r['rows_i']:r['rows_i'] + pj.shape[0]] = pj
        cross, fwd_cpass = r['rows_i'], r['cpass']
        mf_fwd, mf_bwd, mf_bwd_real, _ = _mfma_counts('cross', r['rows_i'], r['rows_j'])
    return dict(pos=rows, nrows=int(rows.shape[0]), cross=int(cross), mp=r['mp'], mirror=0, cpass=r['cpass'], fwd_cpass=fwd_cpass,
                mf_fwd=mf_fwd, mf_bwd=mf_bwd, mf_bwd_real=mf_bwd_real, self_pos=self_pos, mf_self=mf_self,
                direct=torch.as_tensor(r['direct'].reshape(-1), device=dev), conj=torch.as_tensor(r['conj'].reshape(-1), device=dev))


def _two_pass_mask(blocks, raw, Nbl, dev):
    """float32 (Nbl, 1, 1, 1): 1 on the baseline slots of the blocks of a list whose complex forward takes one pass per real
    plane (fwd_cpass == 0), 0 on the slots of its single-pass blocks.  The slots are read from the host tables `raw` of the
    plain blocks: a derived form holds exactly the slots of its plain block (_assert_slots_once)."""
    mask = torch.zeros(Nbl, 1, 1, 1, dtype=torch.float32, device=dev)
    slots = [r[k][r[k] >= 0] for b, r in zip(blocks, raw) if b['fwd_cpass'] == 0 for k in ('direct', 'conj')]
    if slots:
        mask[torch.as_tensor(np.concatenate(slots), dtype=torch.int64, device=dev)] = 1.0
    return mask


def _symmetric_forms(blocks, raw, posh, plan, dev, Nbl):
    """
    The keys that point symmetry adds to geom.ant ({}: no block has a symmetric form).  The REAL-psky passes run every block
    on the first form it has (blocks_real): the pair cross form between the symmetric groups of a larger array (`plan`,
    _pair_cross_plan), the conjugate-pair form, which does not contract the mirror rows either, the mirror form (conjugate
    phasors are not evaluated twice; blocks_mirror), the plain block.  Complex psky keeps the plain blocks (their single-pass
    forms depend on the pair orientation, which a re-ordering of the rows changes) except where a block has a pair form: two
    real passes of that (blocks_cplx).
    """
    mirror, real, cplx, mirror_groups, pair_blocks, pair_cross_blocks = [], [], [], [], [], []
    for b, r in zip(blocks, raw):
        m = q = None
        if r['ants_j'] is not None:
            if plan is not None:
                q = _pair_cross_block(b, plan['cross'][(min(r['gi'], r['gj']), max(r['gi'], r['gj']))], dev)
                pair_cross_blocks.append((q['rows_i'], q['rows_j']))
        else:
            P, host = posh[np.asarray(r['ants_i'])], (r['direct'], r['conj'])
            m, q = _mirror_block(b, P, dev, host), (_pair_block(b, P, dev, host) if PAIR else None)
            if q is not None:
                pair_blocks.append((sum(1 for x in q['partner'] if x >= 0), q['nrows'], int(q['hub'] is not None)))
            elif m is not None:
                mirror_groups.append((bin(m['mirror']).count('1'), (m['nrows'] + 15) // 16))
        mirror.append(b if m is None else m)
        real.append(mirror[-1] if q is None else q)
        cplx.append(b if q is None else q)
    if all(x is b for x, b in zip(mirror + real, blocks + blocks)):
        return {}
    forms = dict(blocks_mirror=mirror, blocks_real=real, mirror_groups=mirror_groups, pair_blocks=pair_blocks)
    if plan is not None:
        forms['pair_cross_blocks'] = pair_cross_blocks
    if PAIR_CPLX and (pair_blocks or pair_cross_blocks):
        forms.update(blocks_cplx=cplx, two_pass_mask_cplx=_two_pass_mask(cplx, raw, Nbl, dev))
    return forms


def _fringe_algorithmic_bytes(geom, a, b):
    """HBM bytes a fused fringe sum cannot avoid: psky (or gpsky) once, the visibilities (or their
    gradient) once, the pointing vectors once -- both directions move the same tensors"""
    return int(a.numel() * a.element_size() + b.numel() * b.element_size() + geom.sdir.numel() * geom.sdir.element_size())


def _fringe_call(geom, backward, inp, out, Npp, cplx, strides=None):
    if geom.ant is not None and inp.dtype == torch.float32 and strides is not None:
        with _timed('fringe_ant_bwd_kernel' if backward else 'fringe_ant_fwd_kernel', geom.elements) as late:
            flops = _fringe_ant_call(geom, backward, inp, out, strides, Npp, cplx)
            if late is not None:
                late += (flops, _fringe_algorithmic_bytes(geom, inp, out))
        return
    code, rdt = _real_dtype(inp)
    fn = lib.rime_fringe_sum_bwd if backward else lib.rime_fringe_sum_fwd
    ws, nbytes = _workspace(lib.rime_fringe_sum_workspace(code, geom.Nbl, geom.Nt, geom.Nf, geom.Pstride,
                                                          geom.Nmp, Npp, int(cplx), int(backward)), inp.device, 16)
    uniform = int(geom.uniform)
    if uniform == 2 and code == RIME_F64 and geom.nu_phi >= NU_F64_PHI:
        uniform = 0
    with _timed('fringe_bwd_kernel' if backward else 'fringe_fwd_kernel', geom.elements, 0) as late:
        rc = fn(code, _ptr(geom.blvecs), _ptr(geom.sdir), _ptr(geom.freqs), _ptr(inp),
                geom.mp_offsets, _ptr(geom.bl_order), geom.Nbl, geom.Nt, geom.Nf, geom.Pstride,
                geom.Nmp, Npp, int(cplx), geom.sign, uniform, geom.f0, geom.df,
                geom.max_blen, strides, _ptr(out), _ptr(ws), nbytes, _stream())
        check(rc, 'rime_fringe_sum_bwd' if backward else 'rime_fringe_sum_fwd')
        if late is not None:
            late.append(_fringe_algorithmic_bytes(geom, inp, out))


def _npp_chunks(Npp, cplx):
    """polarisation-product planes in runs the baseline-formulation kernels take natively (real psky: 4, 2, 1
    planes per launch; complex: 4 or 1): imaging puts any number of maps on this axis"""
    sizes = (4, 1) if cplx else (4, 2, 1)
    out, q = [], 0
    while q < Npp:
        n = next(k for k in sizes if k <= Npp - q)
        out.append((q, n))
        q += n
    return out


def _fringe_call_planes(geom, backward, psky_like, vis_like, cplx):
    """_fringe_call over a psky-shaped tensor (Nt, Nmp, Npp, Nf, P) and a vis-shaped tensor (Npp, Nbl, Nt, Nf):
    one launch when the kernels take the plane count as it is, else one per run of planes"""
    Npp = psky_like.shape[2]
    native = (geom.ant is not None and psky_like.dtype in (torch.float32, torch.complex64)) or \
        (Npp in (1, 4)) or (Npp == 2 and not cplx)
    for q0, n in ([(0, Npp)] if native else _npp_chunks(Npp, cplx)):
        p = psky_like.narrow(2, q0, n)
        v = vis_like.narrow(0, q0, n)
        pr, vr = (torch.view_as_real(p) if cplx else p), torch.view_as_real(v)
        if backward:
            _fringe_call(geom, True, vr, pr, n, cplx, _dense_strides(p))
        else:
            _fringe_call(geom, False, pr, vr, n, cplx, _dense_strides(p))


def _blvec_grad(geom, p, g, cplx):
    """
    d loss / d blvecs [Nbl, 3] of the fringe sum: d vis / d b_k = sum_p psky (sign 2 pi i nu / c) s_k F, i.e. the
    FORWARD kernels on the three direction-cosine-weighted copies of psky (telescope_model.py:350-356 is
    differentiable w.r.t. blvecs through torch autograd; here it costs three more forward passes and is only
    computed when the baseline vectors require a gradient).  p: psky (Nt, Nmp, Npp, Nf, Ps); g: gvis (Npp, Nbl, Nt, Nf).
    """
    Nt, Nmp, Npp, Nf, Ps = p.shape
    rdt = torch.float32 if p.dtype in (torch.float32, torch.complex64) else torch.float64
    s3 = geom.sdir.to(rdt)                                                   # (Nt, 3, Ps)
    pw = (p[:, :, :, None] * s3[:, None, None, :, None, :]).reshape(Nt, Nmp, Npp * 3, Nf, Ps).contiguous()
    w = torch.empty((Npp * 3, geom.Nbl, Nt, Nf), dtype=g.dtype, device=g.device)
    _fringe_call_planes(geom, False, pw, w, cplx)
    w = w.reshape(Npp, 3, geom.Nbl, Nt, Nf)
    fac = (geom.sign * 2.0 * np.pi / 2.99792458e8) * geom.freqs                # (Nf,) float64
    # Re( conj(g) * i fac * w ) = -fac * Im( conj(g) w )
    t = (g.conj()[:, None] * w).imag.to(torch.float64) * (-fac)
    return t.sum(dim=(0, 3, 4)).t().contiguous()                             # (Nbl, 3)


class _FringeSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, psky, geom, blvecs=None):
        _require_cuda(psky)
        assert psky.dim() == 5, 'psky must be (Nt, Nmp, Npp, Nf, Pstride)'
        Nt, Nmp, Npp, Nf, Ps = psky.shape
        assert (Nt, Nmp, Nf, Ps) == (geom.Nt, geom.Nmp, geom.Nf, geom.Pstride), \
            'psky %s does not match geometry (Nt=%d, Nmp=%d, Nf=%d, Pstride=%d)' % (
                tuple(psky.shape), geom.Nt, geom.Nmp, geom.Nf, geom.Pstride)
        cplx = psky.is_complex()
        p = psky.detach()
        strides = _dense_strides(p)          # permuted (e.g. time-inner) layouts are read in place
        if strides is None:
            p = p.contiguous()
            strides = _dense_strides(p)
        _, rdt = _real_dtype(p)
        cdt = torch.complex64 if rdt == torch.float32 else torch.complex128
        vis = torch.empty((Npp, geom.Nbl, Nt, Nf), dtype=cdt, device=p.device)
        _fringe_call_planes(geom, False, p, vis, cplx)
        ctx.geom, ctx.cplx, ctx.dtype = geom, cplx, psky.dtype
        ctx.pshape, ctx.pstride = tuple(p.shape), tuple(p.stride())   # gradient buffer template only
        ctx.psky = p if (blvecs is not None and blvecs.requires_grad) else None     # kept only for the blvecs gradient
        return vis

    @staticmethod
    def backward(ctx, gvis):
        geom = ctx.geom
        g = gvis.contiguous()
        gp = None
        if ctx.needs_input_grad[0]:
            gp = torch.empty_strided(ctx.pshape, ctx.pstride, dtype=ctx.dtype, device=g.device)
            _fringe_call_planes(geom, True, gp, g, ctx.cplx)
        gb = None
        if len(ctx.needs_input_grad) > 2 and ctx.needs_input_grad[2] and ctx.psky is not None:
            gb = _blvec_grad(geom, ctx.psky, g, ctx.cplx)
        return gp, None, gb


def fringe_sum(psky, geom, blvecs=None):
    """
    psky (Nt, Nmp, Npp, Nf, Pstride) real or complex on the GPU; geom a FringeGeometry.
    Returns vis (Npp, Nbl, Nt, Nf) complex.  Differentiable w.r.t. psky and, when `blvecs` -- the (Nbl, 3)
    tensor the geometry was built from, still attached to its graph -- requires a gradient, w.r.t. the baseline
    vectors (hence antenna positions): three extra forward passes in the backward.
    """
    if blvecs is not None and blvecs.requires_grad:
        assert tuple(blvecs.shape) == (geom.Nbl, 3)
        return _FringeSum.apply(psky, geom, blvecs)
    return _FringeSum.apply(psky, geom)


# RIME_FRINGE_MERGE=0: the sky components of a RIME call keep one fringe launch sequence each (A/B measurements)
FRINGE_MERGE = _env_int('RIME_FRINGE_MERGE', 1) != 0
MAX_SEGMENTS = 4


def _merged_block(pskys, geoms):
    """
    The pair block that all components of a fringe_sum_components call run on, or None where they keep their own launches:
    two to four real float32 planes on ONE conjugate-pair block (the same tables: geometries built with ant_like), the same
    baselines, times, channels and fringe sign, one beam-model pair.  Anything else -- generic, packed or cross blocks, a
    complex psky, other dtypes -- is not merged.
    """
    if not FRINGE_MERGE or not 2 <= len(geoms) <= MAX_SEGMENTS:
        return None
    g0, blk = geoms[0], None
    for p, g in zip(pskys, geoms):
        if g.ant is None or p.dtype != torch.float32 or p.dim() != 5 or g.Nmp != 1 or p.shape[2] != pskys[0].shape[2]:
            return None
        blocks = g.ant.get('blocks_real', g.ant['blocks'])
        if len(blocks) != 1 or not blocks[0].get('pair') or blocks[0].get('xpair') or (blk is not None and blocks[0] is not blk):
            return None
        blk = blocks[0]
        if (g.Nbl, g.Nt, g.Nf, g.sign) != (g0.Nbl, g0.Nt, g0.Nf, g0.sign):
            return None
        if tuple(p.shape) != (g.Nt, 1, p.shape[2], g.Nf, g.Pstride):
            return None
        if g is not g0:
            same = g.__dict__.get('_same_freqs')               # compared once per pair of geometries (a device sync)
            if same is None or same[0] is not g0.freqs:
                same = g.__dict__['_same_freqs'] = (g0.freqs, bool(torch.equal(g.freqs, g0.freqs)))
            if not same[1]:
                return None
    return blk


def _segment_table(geoms, planes, pp, backward, scales=None, accumulate=0):
    """rime_fringe_segment array of the planes `pp` of (Nt, 1, Npp, Nf, Ps) float32 tensors with a contiguous pixel axis"""
    segs = (_lib.FringeSegment * len(geoms))()
    for s, g, p in zip(segs, geoms, planes):
        st = p.stride()
        s.sdir, s.Pstride, s.st_t, s.st_f, s.st_p = g.sdir.data_ptr(), g.Pstride, max(st[0], 1), max(st[3], 1), 1
        plane = p.data_ptr() + 4 * pp * st[2]
        if backward:
            s.gpsky, s.accumulate = plane, accumulate
        else:
            s.psky = plane
    if scales is not None:
        for s, (scale, rowmin) in zip(segs, scales):
            s.scale, s.rowmin = scale[0, pp].data_ptr(), rowmin[0, pp].data_ptr()
    return segs


def _merged_call(blk, geoms, backward, planes, vis_real):
    """
    One pair launch per direction over the segment table of the components (csrc/fringe_mfma.hip, SEGMENTS).  Forward:
    planes = the psky of every component, vis_real (Npp, Nbl, Nt, Nf, 2) is written.  Backward: planes = the gradient buffers
    of the components that need one (geoms alike), vis_real the gradient of the visibilities: ONE transpose and ONE row scale
    of it serve all of them.  Recorded in PROFILE under the family names of the per-component calls (below).
    """
    g0 = geoms[0]
    Nbl, Nt, Nf, Npp, dev = g0.Nbl, g0.Nt, g0.Nf, planes[0].shape[2], planes[0].device
    name, lead, tables, _, mf = _block_launch(blk, backward, 0)
    name = name.replace('_block', '_segments')
    Ps = (ctypes.c_int * len(geoms))(*[g.Pstride for g in geoms])
    family = 'fringe_ant_bwd_kernel' if backward else 'fringe_ant_fwd_kernel'
    vbytes = vis_real.numel() * vis_real.element_size()
    work = [(g.elements, mf * Npp * Nt * Nf * (g.Pstride // 16) * 32768,
             int(p.numel() * p.element_size() + vbytes + g.sdir.numel() * g.sdir.element_size())) for p, g in zip(planes, geoms)]
    prof = PROFILE
    with _timed(family, work[0][0]) as late:
        if not backward:
            scales = []
            for p in planes:
                scale = torch.empty((1, Npp, Nt, Nf), dtype=torch.float32, device=dev)
                rowmin = torch.empty_like(scale)
                check(lib.rime_fringe_row_scale(_ptr(p), 1, Npp, Nt, Nf, p.stride(1), p.stride(2), p.stride(0), p.stride(3),
                                                p.shape[-1], _ptr(scale), _ptr(rowmin), _stream()), 'rime_fringe_row_scale')
                scales.append((scale, rowmin))
            ws, nbytes = _workspace(lib.rime_fringe_pair_segments_workspace(Nbl, Nt, Nf, Ps, len(geoms)), dev, 16)
            for pp in range(Npp):
                segs = _segment_table(geoms, planes, pp, False, scales)
                check(getattr(lib, name)(*lead, _ptr(g0.freqs), *tables, Nbl, Nt, Nf, g0.sign, segs, len(geoms), _ptr(ws), nbytes,
                                         _stream()), name)
                check(lib.rime_fringe_pair_segments_finish(_ptr(ws), nbytes, _ptr(vis_real[pp]), Nbl, Nt, Nf, Ps, len(geoms),
                                                           _stream()), 'rime_fringe_pair_segments_finish')
        else:
            ws, nbytes = _workspace(lib.rime_fringe_ant_bwd_workspace(Nbl, Nt, Nf), dev, 16)
            gvt = ws[:Nt * Nf * 2 * Nbl * 4].view(torch.float32).view(Nt * Nf, 2 * Nbl)
            for pp in range(Npp):
                check(lib.rime_fringe_ant_bwd_prepare(_ptr(vis_real[pp]), Nbl, Nt, Nf, _ptr(ws), nbytes, _stream()),
                      'rime_fringe_ant_bwd_prepare')
                gscale = torch.empty(Nt * Nf, dtype=torch.float32, device=dev)
                check(lib.rime_fringe_row_scale(_ptr(gvt), 1, 1, 1, Nt * Nf, 0, 0, 0, 2 * Nbl, 2 * Nbl, _ptr(gscale), None,
                                                _stream()), 'rime_fringe_row_scale')
                segs = _segment_table(geoms, planes, pp, True)
                check(getattr(lib, name)(*lead, _ptr(g0.freqs), _ptr(gscale), *tables, Nbl, Nt, Nf, g0.sign, segs, len(geoms),
                                         _ptr(ws), nbytes, _stream()), name)
        if late is not None:
            late += work[0][1:]
    if prof is not None:
        # one record per segment under the family name, as the per-component calls leave them: the first holds the time of
        # the whole launch, the others their elements / flops / bytes with an empty interval, so sums over the family hold
        for w in work[1:]:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            prof.append((family, e, e) + w)


class _FringeSumMerged(torch.autograd.Function):
    """sum over sky components of fringe_sum(psky_k, geom_k), one node: N psky inputs, N gradients"""
    @staticmethod
    def forward(ctx, blk, geoms, *pskys):
        _require_cuda(*pskys)
        planes = []
        for p in pskys:
            p = p.detach()
            planes.append(p if _dense_strides(p) is not None else p.contiguous())
        g0 = geoms[0]
        vis = torch.empty((planes[0].shape[2], g0.Nbl, g0.Nt, g0.Nf), dtype=torch.complex64, device=planes[0].device)
        _merged_call(blk, geoms, False, planes, torch.view_as_real(vis))
        ctx.blk, ctx.geoms = blk, geoms
        ctx.templates = [(tuple(p.shape), tuple(p.stride())) for p in planes]
        return vis

    @staticmethod
    def backward(ctx, gvis):
        g = gvis.contiguous()
        need = [k for k in range(len(ctx.geoms)) if ctx.needs_input_grad[2 + k]]
        grads = [None] * len(ctx.geoms)
        if need:
            for k in need:
                shape, stride = ctx.templates[k]
                grads[k] = torch.empty_strided(shape, stride, dtype=torch.float32, device=g.device)
            _merged_call(ctx.blk, [ctx.geoms[k] for k in need], True, [grads[k] for k in need], torch.view_as_real(g))
        return (None, None) + tuple(grads)


def fringe_sum_components(pskys, geoms, blvecs=None):
    """
    sum_k fringe_sum(pskys[k], geoms[k]): the visibilities of several sky components seen by one array at the same times and
    channels (RIME.forward).  Where every component runs on the same conjugate-pair block this is ONE launch per direction
    over a segment table, one reduction of the slabs and, in the backward, one transpose and row scale of the gradient;
    otherwise (and with RIME_FRINGE_MERGE=0, or a blvecs that requires a gradient) the per-component calls, added up.
    A component whose psky does not require a gradient takes no part in the backward launch.
    """
    pskys, geoms = list(pskys), list(geoms)
    assert len(pskys) == len(geoms) and pskys
    blk = None if (blvecs is not None and blvecs.requires_grad) else _merged_block(pskys, geoms)
    if blk is not None:
        return _FringeSumMerged.apply(blk, geoms, *pskys)
    vis = None
    for p, g in zip(pskys, geoms):
        v = fringe_sum(p, g, blvecs)
        vis = v if vis is None else vis + v
    return vis


def fringe_adjoint(gvis, geom, Npp=None, dtype=None):
    """
    The adjoint of fringe_sum for a REAL psky, without autograd:  out[t, 0, q, f, p] = Re sum_b
    conj(F[b, t, f, p]) gvis[q, b, t, f] -- the map-making direction (visibilities -> pixels,
    imaging.make_map).  gvis (Npp, Nbl, Nt, Nf) complex; returns (Nt, 1, Npp, Nf, Pstride) real.
    """
    _require_cuda(gvis)
    assert gvis.is_complex() and gvis.dim() == 4 and geom.Nmp == 1
    g = gvis.detach().contiguous()
    Npp = g.shape[0] if Npp is None else Npp
    assert tuple(g.shape) == (Npp, geom.Nbl, geom.Nt, geom.Nf)
    rdt = torch.float32 if g.dtype == torch.complex64 else torch.float64
    out = torch.empty((geom.Nt, 1, Npp, geom.Nf, geom.Pstride), dtype=rdt, device=g.device)
    _fringe_call_planes(geom, True, out, g, False)
    return out


def gen_fringe(blvecs, sdir, freqs, conj=False, dtype=torch.float32):
    """materialised fringe (Nbl, Nf, P) complex; blvecs (Nbl,3), sdir (3,P) float64 on the GPU"""
    _require_cuda(blvecs, sdir)
    b = blvecs.detach().to(torch.float64).contiguous()
    s = sdir.detach().to(torch.float64).contiguous()
    f = torch.as_tensor(freqs, dtype=torch.float64).to(b.device).contiguous()
    cdt = torch.complex64 if dtype == torch.float32 else torch.complex128
    out = torch.empty((b.shape[0], len(f), s.shape[1]), dtype=cdt, device=b.device)
    rc = lib.rime_gen_fringe(RIME_F32 if dtype == torch.float32 else RIME_F64, _ptr(b), _ptr(s), _ptr(f),
                             b.shape[0], len(f), s.shape[1], s.shape[1], -1 if conj else 1,
                             _ptr(torch.view_as_real(out)), _stream())
    check(rc, 'rime_gen_fringe')
    return out


def eq2top(ra, dec, M, vbary, vdiurnal):
    """
    ICRS (ra, dec) [deg, float64 on the GPU] -> (2, N) float64 tensor (zen, az) [deg]: annual
    aberration, rotation by the host-built matrix M (3, 3) (ICRS -> East, North, Up), diurnal
    aberration (astrometry.observation_frame gives M, vbary, vdiurnal per observation time).
    """
    _require_cuda(ra, dec)
    r = ra.detach().to(torch.float64).contiguous()
    d = dec.detach().to(torch.float64).contiguous()
    assert r.dim() == 1 and r.shape == d.shape
    out = torch.empty((2, r.numel()), dtype=torch.float64, device=r.device)
    Mh = (ctypes.c_double * 9)(*[float(x) for x in np.asarray(M, dtype=np.float64).reshape(-1)])
    vh = (ctypes.c_double * 3)(*[float(x) for x in np.asarray(vbary, dtype=np.float64).reshape(-1)])
    rc = lib.rime_eq2top(_ptr(r), _ptr(d), r.numel(), ctypes.cast(Mh, ctypes.c_void_p), ctypes.cast(vh, ctypes.c_void_p),
                         float(vdiurnal), _ptr(out[0]), _ptr(out[1]), _stream())
    check(rc, 'rime_eq2top')
    return out


# ---------------------------------------------------------------------------------------
class _JonesApply(torch.autograd.Function):
    """psky[a, d] = sum_bc J1[a, b] S[b, c] conj(J2[d, c]) in one pass (csrc/jones.hip); J2 is J1 when `same`"""
    @staticmethod
    def forward(ctx, J1, J2, S, same):
        _require_cuda(J1, J2, S)
        j1 = J1.detach().contiguous()
        j2 = j1 if same else J2.detach().contiguous()
        sk = S.detach().contiguous()
        assert sk.is_complex() and tuple(j1.shape[:2]) == (2, 2) and tuple(sk.shape[:2]) == (2, 2) and j1.shape == j2.shape
        assert j2.dtype == j1.dtype, 'both Jones operands must have one dtype (%s vs %s)' % (j1.dtype, j2.dtype)
        code, rdt = _real_dtype(sk)
        bc = j1.is_complex()
        assert (j1.dtype == sk.dtype) if bc else (j1.dtype == rdt), 'beam %s vs sky %s' % (j1.dtype, sk.dtype)
        N, Ns = j1[0, 0].numel(), sk[0, 0].numel()
        assert N % Ns == 0 and tuple(j1.shape[-2:]) == tuple(sk.shape[-2:])
        out = torch.empty(j1.shape, dtype=sk.dtype, device=sk.device)
        vr = torch.view_as_real
        rc = lib.rime_jones_apply_fwd(code, int(bc), _ptr(vr(j1) if bc else j1), _ptr(vr(j2) if bc else j2), _ptr(vr(sk)),
                                      N, Ns, _ptr(vr(out)), _stream())
        check(rc, 'rime_jones_apply_fwd')
        ctx.save_for_backward(j1, j2, sk)
        ctx.same, ctx.sky_shape = same, tuple(S.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        j1, j2, sk = ctx.saved_tensors
        g = g.contiguous()
        code, _ = _real_dtype(sk)
        bc = j1.is_complex()
        N, Ns = j1[0, 0].numel(), sk[0, 0].numel()
        g1, g2 = torch.empty_like(j1), torch.empty_like(j1)
        gs = torch.empty(j1.shape, dtype=sk.dtype, device=sk.device)
        vr = torch.view_as_real
        rc = lib.rime_jones_apply_bwd(code, int(bc), _ptr(vr(j1) if bc else j1), _ptr(vr(j2) if bc else j2), _ptr(vr(sk)),
                                      _ptr(vr(g)), N, Ns, _ptr(vr(g1) if bc else g1), _ptr(vr(g2) if bc else g2),
                                      _ptr(vr(gs)), _stream())
        check(rc, 'rime_jones_apply_bwd')
        if N != Ns:                                       # one sky for several model pairs: sum their contributions
            gs = gs.reshape(2, 2, N // Ns, Ns).sum(2)
        gs = gs.reshape(ctx.sky_shape)
        if ctx.same:
            return g1 + g2, None, gs, None
        return g1, g2, gs, None


def jones_apply(J1, J2, S):
    """
    Full-polarisation beam x sky product J1 S J2^dagger per pixel, channel and beam-model pair (the 4-pol branch of
    PixelBeam.apply_beam, beam_model.py:345-363).  J1, J2 (2, 2, Nmp, Nf, P) real or complex (J2 may be J1 itself),
    S (2, 2, 1 | Nmp, Nf, P) complex -> (2, 2, Nmp, Nf, P) complex.
    """
    return _JonesApply.apply(J1, J2, S, J2 is J1)


class _Stokes2Coh(torch.autograd.Function):
    """C = I [[1 + fQ, fU - i fV], [fU + i fV, 1 - fQ]] in one pass each way (csrc/jones.hip); fractions without gradient"""
    @staticmethod
    def forward(ctx, I, frb):
        _require_cuda(I, frb)
        x = I.detach().contiguous()
        code, rdt = _real_dtype(x)
        cdt = torch.complex64 if rdt == torch.float32 else torch.complex128
        P = x.shape[-1]
        R = x.numel() // P
        out = torch.empty((2, 2) + tuple(x.shape), dtype=cdt, device=x.device)
        # frb: (3,) + I.shape expanded view of the fractions: element strides, 0 on broadcast axes; rows must share ONE stride
        fs = _frac_strides(frb, x.shape)
        check(lib.rime_stokes2coh_fwd(code, _ptr(x), _ptr(frb), fs[0], fs[1], fs[2], R, P, _ptr(torch.view_as_real(out)), _stream()),
              'rime_stokes2coh_fwd')
        ctx.frb, ctx.fs, ctx.shape, ctx.code = frb, fs, tuple(I.shape), code
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        P = ctx.shape[-1]
        R = int(np.prod(ctx.shape[:-1])) if len(ctx.shape) > 1 else 1
        gI = torch.empty(ctx.shape, dtype=ctx.frb.dtype, device=g.device)
        check(lib.rime_stokes2coh_bwd(ctx.code, _ptr(torch.view_as_real(g)), _ptr(ctx.frb), ctx.fs[0], ctx.fs[1], ctx.fs[2], R, P,
                                      _ptr(gI), _stream()), 'rime_stokes2coh_bwd')
        return gI, None


def _frac_strides(frb, shape):
    """(fs_k, fs_r, fs_p) element strides of an expanded (3,) + shape view, or None when the leading axes of `shape` cannot
    be addressed by one row stride (then the caller keeps the torch composition)"""
    st = frb.stride()
    fs_p = st[-1] if shape[-1] > 1 else 0
    lead, lst = list(shape[:-1]), list(st[1:-1])
    # rows r = flattened leading axes: one stride only if the axes are jointly contiguous or all broadcast
    live = [(n, s_) for n, s_ in zip(lead, lst) if n > 1]
    if not live or all(s_ == 0 for _, s_ in live):
        fs_r = 0
    else:
        fs_r = live[-1][1]
        acc = fs_r
        for n, s_ in reversed(live):
            if s_ != acc:
                return None
            acc *= n
    return (st[0], fs_r, fs_p)


def stokes2coherency(I, frac):
    """
    Stokes I map (..., Npix) real on the GPU + fractional polarisation `frac` (3, 1, ...) broadcastable to (3,) + I.shape
    (fQ, fU, fV) -> coherency (2, 2, ..., Npix) complex (sky_model.Stokes2Coherency's Stokes-I branch, sky_model.py:1160-1300)
    in one fused pass; differentiable w.r.t. I.  Returns None when the layout is not served (fractions that require a
    gradient, another dtype, leading axes without a common stride): the caller keeps the torch composition.
    """
    if not (I.is_cuda and I.dtype in (torch.float32, torch.float64) and not I.is_complex()):
        return None
    if frac.requires_grad or frac.dtype != I.dtype or frac.shape[0] != 3 or frac.device != I.device:
        return None
    # axis 1 of `frac` is the singleton the reference keeps there; the axes behind it must line up ONE TO ONE with I's (a frac
    # with fewer trailing axes would be left-padded by expand and could land its Q/U/V axis on I's channel axis: ADVICE r04)
    if frac.dim() - 2 != I.dim() or frac.shape[1] != 1:
        return None
    try:
        frb = frac.detach().reshape((3,) + tuple(frac.shape[2:])).expand((3,) + tuple(I.shape))
    except RuntimeError:
        return None
    if _frac_strides(frb, tuple(I.shape)) is None or any(s_ < 0 for s_ in frb.stride()):
        return None
    return _Stokes2Coh.apply(I, frb)


# ---------------------------------------------------------------------------------------
class InterpStencil:
    """(inds, wgts) of PixInterp plus the CSR inverse index the deterministic adjoint uses."""
    def __init__(self, inds, wgts, Npb):
        _require_cuda(inds, wgts)
        self.P, self.Nnn = inds.shape
        self.Npb = int(Npb)
        self.inds = inds.to(torch.int32).contiguous()
        self.wgts = wgts.contiguous()
        flat = self.inds.reshape(-1).to(torch.int64)
        # entries of weight 0 (the padding slots of a one-node FoV-cut stencil all point at the last pixel; samples on a
        # grid node) stay out of the inverse index: the gather skips them too (w != 0), so 0 * inf / NaN of a padded
        # gradient slot cannot reach the map gradient, and no node collects thousands of dead entries for one wave to walk
        keep = torch.nonzero(self.wgts.reshape(-1) != 0).reshape(-1)
        order = keep[torch.sort(flat[keep], stable=True).indices]
        counts = torch.bincount(flat[keep], minlength=self.Npb)
        ptr = torch.zeros(self.Npb + 1, dtype=torch.int64, device=inds.device)
        ptr[1:] = torch.cumsum(counts, 0)
        self.csr_ptr = ptr.to(torch.int32).contiguous()
        self.csr_src = order.to(torch.int32).contiguous()
        self._wcache = {self.wgts.dtype: self.wgts}

    def weights(self, dtype):
        if dtype not in self._wcache:
            self._wcache[dtype] = self.wgts.to(dtype).contiguous()
        return self._wcache[dtype]


class _InterpGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, m, st, out_stride):
        _require_cuda(m)
        lead = m.shape[:-1]
        Npb = m.shape[-1]
        assert Npb == st.Npb, 'map has %d pixels, stencil was built for %d' % (Npb, st.Npb)
        cplx = m.is_complex()
        mm = m.detach().contiguous()
        code, rdt = _real_dtype(mm)
        R = int(np.prod(lead)) if len(lead) else 1
        out = torch.zeros(lead + (out_stride,), dtype=m.dtype, device=m.device)
        rc = lib.rime_interp_gather_fwd(code, int(cplx), _ptr(torch.view_as_real(mm) if cplx else mm),
                                        _ptr(st.inds), _ptr(st.weights(rdt)), R, Npb, st.P, st.Nnn,
                                        _ptr(torch.view_as_real(out) if cplx else out), out_stride,
                                        _stream())
        check(rc, 'rime_interp_gather_fwd')
        ctx.st, ctx.shape, ctx.cplx, ctx.out_stride = st, tuple(m.shape), cplx, out_stride
        return out

    @staticmethod
    def backward(ctx, gout):
        st = ctx.st
        code, rdt = _real_dtype(gout)
        R = int(np.prod(ctx.shape[:-1])) if len(ctx.shape) > 1 else 1
        if st.Nnn == 1:
            # one-node stencil (FoV cut, redundant inflation): row-major adjoint, no transposed copies, and the gradient that
            # goes upstream is contiguous
            g = gout.contiguous()
            gm = torch.empty(ctx.shape, dtype=gout.dtype, device=gout.device)
            rc = lib.rime_interp_scatter_rows_bwd(code, int(ctx.cplx), _ptr(torch.view_as_real(g) if ctx.cplx else g),
                                                  ctx.out_stride, _ptr(st.csr_ptr), _ptr(st.csr_src), _ptr(st.weights(rdt)),
                                                  R, st.Npb, _ptr(torch.view_as_real(gm) if ctx.cplx else gm), _stream())
            check(rc, 'rime_interp_scatter_rows_bwd')
            return gm, None, None
        if st.csr_src.numel() == 0:                      # every weight 0: nothing reaches the map
            return torch.zeros(ctx.shape, dtype=gout.dtype, device=gout.device), None, None
        # transposed working layout [pixel][row]: every read / write of the kernel is coalesced
        gT = gout.reshape(R, ctx.out_stride)[:, :st.P].t().contiguous()
        gmT = torch.empty((st.Npb, R), dtype=gout.dtype, device=gout.device)
        rc = lib.rime_interp_scatter_bwd(code, int(ctx.cplx),
                                         _ptr(torch.view_as_real(gT) if ctx.cplx else gT),
                                         _ptr(st.csr_ptr), _ptr(st.csr_src), _ptr(st.weights(rdt)),
                                         R, st.Npb, st.P, st.Nnn,
                                         _ptr(torch.view_as_real(gmT) if ctx.cplx else gmT), _stream())
        check(rc, 'rime_interp_scatter_bwd')
        return gmT.t().contiguous().reshape(ctx.shape), None, None


def interp_gather(m, stencil, out_stride=None):
    """out[..., p] = sum_k w[p,k] m[..., inds[p,k]]; columns P..out_stride are zero padding."""
    return _InterpGather.apply(m, stencil, stencil.P if out_stride is None else int(out_stride))


class _NodeMajor(torch.autograd.Function):
    """(R, Npix_beam) beam map -> node-major (Npix_beam, R) copy, the layout the fused psky builder gathers from (a node's value
    for 4 channels is one vector load), as an autograd node of its own: a forward with several sky components (C4: diffuse +
    point sources) transposes the map ONCE, and the components' node-major gradients are summed before the ONE transposition
    back (round 5: one 34-MB transposing copy less each way per C4 step)"""
    @staticmethod
    def forward(ctx, bmap):
        return bmap.detach().t().contiguous()

    @staticmethod
    def backward(ctx, g):
        # one explicit transposition: everything upstream (the |.| of a power beam, the accumulation into .grad) then runs on a
        # contiguous tensor instead of a transposed view
        return g.t().contiguous()


def node_major(bmap):
    return _NodeMajor.apply(bmap)


class _BeamSkyProduct(torch.autograd.Function):
    """psky[r, q] = interp(bmap)[r, q] * sky[r, cut[q]] in one pass (see rime_beam_sky_fwd); bmapT = the NODE-MAJOR map"""
    @staticmethod
    def forward(ctx, bmapT, sky, st, cut, pos, Nt, Ps):
        _require_cuda(bmapT, sky)
        Npb, R = bmapT.shape
        Npix = sky.shape[1]
        assert sky.shape[0] == R and Npb == st.Npb and st.P == Nt * Ps and bmapT.dtype == sky.dtype
        b, k = bmapT.detach().contiguous(), sky.detach().contiguous()
        code, rdt = _real_dtype(b)
        out = torch.empty((R, Nt * Ps), dtype=b.dtype, device=b.device)
        rc = lib.rime_beam_sky_fwd(code, _ptr(b), _ptr(k), _ptr(st.inds), _ptr(st.weights(rdt)), _ptr(cut),
                                   R, Npb, Npix, Nt * Ps, st.Nnn, _ptr(out), _stream())
        check(rc, 'rime_beam_sky_fwd')
        ctx.save_for_backward(b, k)
        ctx.aux = (st, cut, pos, Nt, Ps)
        return out

    @staticmethod
    def backward(ctx, g):
        b, k = ctx.saved_tensors
        st, cut, pos, Nt, Ps = ctx.aux
        Npb, R = b.shape
        Npix = k.shape[1]
        Q = Nt * Ps
        code, rdt = _real_dtype(b)
        g = g.contiguous()
        T1 = torch.empty((Q, R), dtype=b.dtype, device=b.device)
        gsky = torch.empty((R, Npix), dtype=b.dtype, device=b.device)
        ws, nws = _workspace(lib.rime_beam_sky_bwd_workspace(code, R, Npix, Nt), b.device)
        rc = lib.rime_beam_sky_bwd(code, _ptr(g), _ptr(b), _ptr(k), _ptr(st.inds), _ptr(st.weights(rdt)), _ptr(cut),
                                   _ptr(pos), R, Npb, Npix, Nt, Ps, st.Nnn, _ptr(T1), _ptr(gsky), _ptr(ws), nws, _stream())
        check(rc, 'rime_beam_sky_bwd')
        gmT = torch.empty((Npb, R), dtype=b.dtype, device=b.device)
        rc = lib.rime_interp_scatter_bwd(code, 0, _ptr(T1), _ptr(st.csr_ptr), _ptr(st.csr_src), _ptr(st.weights(rdt)),
                                         R, Npb, Q, st.Nnn, _ptr(gmT), _stream())
        check(rc, 'rime_interp_scatter_bwd')
        return gmT, gsky, None, None, None, None, None


def beam_sky_product(bmap, sky, stencil, cut, pos, Nt, Ps, node_major_map=None):
    """
    Fused interpolate-cut-multiply of the 1-pol power-beam case: bmap (R, Npix_beam) and sky (R, Npix)
    real, same dtype; stencil an InterpStencil over the Nt*Ps (padded) pointing angles; cut int32
    (Nt*Ps) sky-pixel index per point (Npix = padding); pos int32 (Nt, Npix) its inverse per time step
    (-1 = not visible).  Returns psky (R, Nt*Ps).  Differentiable w.r.t. bmap and sky.
    `node_major_map`: ops.node_major(bmap) made by the caller (shared by several calls on the same map); bmap is then ignored.
    """
    bT = node_major(bmap) if node_major_map is None else node_major_map
    return _BeamSkyProduct.apply(bT, sky, stencil, cut, pos, int(Nt), int(Ps))


class _Chisq(torch.autograd.Function):
    """chi^2 = sum icov |pred - data|^2 and its backward in one pass each (see rime_chisq_fwd)"""
    @staticmethod
    def forward(ctx, pred, data, icov):
        _require_cuda(pred)
        assert pred.is_complex(), 'prediction must be complex'
        p = pred.detach().contiguous()
        code, rdt = _real_dtype(p)
        d = None if data is None else data.detach().to(p.dtype).expand_as(p).contiguous()
        w = None if icov is None else icov.detach().to(rdt).expand_as(p).contiguous()
        out = torch.empty((), dtype=rdt, device=p.device)
        ws, nws = _workspace(lib.rime_chisq_workspace(), p.device)
        rc = lib.rime_chisq_fwd(code, _cptr(p), _cptr(d), _ptr(w), p.numel(), _ptr(out), _ptr(ws), nws, _stream())
        check(rc, 'rime_chisq_fwd')
        ctx.saved = (p, d, w)
        return out

    @staticmethod
    def backward(ctx, g):
        p, d, w = ctx.saved
        code, rdt = _real_dtype(p)
        gp = torch.empty_like(p)
        gg = g.detach().to(rdt).reshape(1).contiguous()
        rc = lib.rime_chisq_bwd(code, _cptr(p), _cptr(d), _ptr(w), _ptr(gg), p.numel(), _cptr(gp), _stream())
        check(rc, 'rime_chisq_bwd')
        return gp, None, None


def chisq(pred, data=None, icov=None):
    """
    sum_i icov_i |pred_i - data_i|^2 (real scalar) for a complex prediction; data complex or None (0),
    icov real (inverse variance, diagonal) or None (1), both broadcastable to pred.  Differentiable
    w.r.t. pred.  The fused form of LogProb.forward_chisq's residual + apply_icov(cov_axis=None) + sum.
    """
    return _Chisq.apply(pred, data, icov)


# data axis a covariance couples, per (mode, cov_axis); the data are (Npol, Npol, Nbl, Nt, Nf) or (Npol, 1, Nf, Npix)
_COV_AXES = {('vis', 'bl'): 2, ('vis', 'time'): 3, ('vis', 'freq'): 4, ('map', 'freq'): 2, ('map', 'pix'): 3}
ICOV_PLAN_FIELDS = ('lanes', 'vec', 'tile', 'splits', 'rows_per_split', 'grid', 'stage_bytes', 'lds_bytes', 'stage_limit',
                    'tile_along_outer')


def cov_axis_layout(shape, cov_axis, mode='vis'):
    """
    The one mapping of the axis covariances ("Axis covariances"): data of `shape` seen as (O, n, I) with the covariance axis in
    the middle, its inverse covariance as (O I, n, n) with batch index o I + i.  Returns (axis, O, n, I, icov_shape,
    out_shape): the data axis, the three extents, the documented shape of icov (batch axes in data order, then n, n) and the
    shape of the per-batch chi-square (the data's without that axis).  NameError for an unknown cov_axis / mode pair.
    """
    if (mode, cov_axis) not in _COV_AXES:
        raise NameError("didn't recognize cov_axis %r for mode %r" % (cov_axis, mode))
    shape = tuple(int(s) for s in shape)
    if len(shape) != (5 if mode == 'vis' else 4):
        raise ValueError("mode %r takes data of %d axes, got shape %s" % (mode, 5 if mode == 'vis' else 4, shape))
    axis = _COV_AXES[(mode, cov_axis)]
    O, n, I = int(np.prod(shape[:axis], dtype=np.int64)), shape[axis], int(np.prod(shape[axis + 1:], dtype=np.int64))
    out_shape = shape[:axis] + shape[axis + 1:]
    return axis, O, n, I, out_shape + (n, n), out_shape


def icov_plan(dtype, O, n, I):
    """the launch plan of rime_icov_fwd for a shape, as a dict of ICOV_PLAN_FIELDS (no GPU needed); ValueError when n
    is too long for the LDS staging (RIME_EUNSUPPORTED) -- callers then take the torch path"""
    out = (ctypes.c_int * len(ICOV_PLAN_FIELDS))()
    rc = lib.rime_icov_plan(_dtype_code(dtype), int(O), int(n), int(I), out)
    if rc == -4:
        raise ValueError('covariance axis of %d elements does not fit the LDS staging of the fused kernel' % n)
    check(rc, 'rime_icov_plan')
    return dict(zip(ICOV_PLAN_FIELDS, out))


def chisq_axis_fits(shape, dtype, cov_axis, mode='vis'):
    """whether chisq_axis serves data of `shape` and complex `dtype`: False when the covariance axis is too long for the
    kernel's LDS staging -- the one fall-back rule of its callers (no GPU needed)"""
    _, O, n, I, _, _ = cov_axis_layout(shape, cov_axis, mode)
    try:
        icov_plan(dtype, O, n, I)
    except ValueError:
        return False
    return True


def _icov_fwd_call(p, d, w, O, n, I, y, q, out):
    code, _ = _real_dtype(p)
    ws, nws = _workspace(lib.rime_icov_workspace(code, O, n, I), p.device)
    with _timed('icov_fwd_kernel', O * I * n * n):
        rc = lib.rime_icov_fwd(code, _cptr(p), _cptr(d), _cptr(w), O, n, I, _cptr(y), _ptr(q), _ptr(out), _ptr(ws), nws, _stream())
        if rc == -4:
            raise ValueError('covariance axis of %d elements does not fit the LDS staging of the fused kernel' % n)
        check(rc, 'rime_icov_fwd')


class _ChisqAxis(torch.autograd.Function):
    """r^H W r along one data axis and its backward 2 g W r from the saved W r (see rime_icov_fwd)"""
    _warned = False
    @staticmethod
    def forward(ctx, pred, data, icov, cov_axis, mode, sum_chisq, keep):
        _require_cuda(pred, data, icov)
        assert pred.is_complex(), 'prediction must be complex'
        axis, O, n, I, icov_shape, out_shape = cov_axis_layout(pred.shape, cov_axis, mode)
        if tuple(icov.shape) != icov_shape:
            raise ValueError("cov_axis %r, mode %r, data %s: icov must be %s, got %s"
                             % (cov_axis, mode, tuple(pred.shape), icov_shape, tuple(icov.shape)))
        p = _dense(pred)
        code, rdt = _real_dtype(p)
        d = None if data is None else _dense(data.expand_as(p), p.dtype)
        if icov.dtype != p.dtype and not _ChisqAxis._warned:
            _ChisqAxis._warned = True
            warnings.warn('chisq_axis: icov is %s, the prediction %s: the whole inverse covariance is converted on every '
                          'call; store it in the prediction\'s dtype' % (icov.dtype, p.dtype))
        w = _dense(icov, p.dtype)
        if w.data_ptr() % 16:
            w = w.clone()
        y = torch.empty_like(p) if keep else None
        if sum_chisq:
            out = torch.empty((), dtype=rdt, device=p.device)
            _icov_fwd_call(p, d, w, O, n, I, y, None, out)
        else:
            out = torch.empty(out_shape, dtype=rdt, device=p.device)
            _icov_fwd_call(p, d, w, O, n, I, y, out, None)
        ctx.saved = (y, O, n, I, bool(sum_chisq))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        y, O, n, I, summed = ctx.saved
        code, rdt = _real_dtype(y)
        gg = g.detach().to(rdt).reshape(1 if summed else O * I).contiguous()
        gp = torch.empty_like(y)
        rc = lib.rime_icov_bwd(code, _cptr(y), _ptr(gg), int(not summed), O, n, I, _cptr(gp), _stream())
        check(rc, 'rime_icov_bwd')
        return gp, None, None, None, None, None, None


def chisq_axis(pred, data, icov, cov_axis, mode='vis', sum_chisq=True):
    """
    (pred - data)^H icov (pred - data) with an inverse covariance along ONE data axis, on the fused kernel: pred complex,
    (Npol, Npol, Nbl, Nt, Nf) for mode 'vis' or (Npol, 1, Nf, Npix) for 'map'; data complex and broadcastable to pred, or
    None (0); icov complex in the shape optim.apply_icov documents for cov_axis ('bl', 'time', 'freq'; 'freq', 'pix' for a
    map) -- see cov_axis_layout.  icov must be HERMITIAN in its last two axes (it is an inverse covariance): the backward,
    2 g icov (pred - data) from the product the forward saved, relies on it, and nothing checks it.  Returns the real 0-d
    sum, or with sum_chisq=False the real per-batch values in the data's shape without the covariance axis.
    Differentiable w.r.t. pred only: data and icov are constants and must not require grad.  The product icov (pred - data)
    is kept only when pred requires grad.  ValueError when the axis is too long for the kernel's LDS staging
    (chisq_axis_fits).  Store icov in pred's dtype: another dtype is converted whole on every call (warned once).
    """
    for name, t in (('data', data), ('icov', icov)):
        if t is not None and t.requires_grad:
            raise ValueError('chisq_axis is differentiable in pred only: %s requires grad' % name)
    keep = pred.requires_grad and torch.is_grad_enabled()      # read here: grad mode is off inside forward
    return _ChisqAxis.apply(pred, data, icov, cov_axis, mode, bool(sum_chisq), keep)


# ---------------------------------------------------------------------------------------
# full PSF matrix on the fused phasor-Gram kernel (csrc/psf.hip; DESIGN.md, "Full PSF matrix")
# ---------------------------------------------------------------------------------------
PSF_TILE = 64        # rime::PSF_TILE: side of the output tile of one work-group
PSF_BCHUNK = 16      # rime::PSF_BCHUNK: baselines per LDS chunk
PSF_FLUSH = 1024     # rime::PSF_FLUSH: baselines between two flushes of the accumulators


def _psf_index(idx, n, extent, name, device):
    """an index map of psf_gram as int32 on the device: n unique entries in [0, extent); None stays None"""
    if idx is None:
        return None
    idx = torch.as_tensor(idx, device=device)
    if idx.dtype not in (torch.int32, torch.int64) or idx.ndim != 1 or idx.numel() != n:
        raise ValueError('%s must be %d integer indices, got %s %s' % (name, n, idx.dtype, tuple(idx.shape)))
    if n and (int(idx.min()) < 0 or int(idx.max()) >= extent):
        raise ValueError('%s has an index outside [0, %d)' % (name, extent))
    if torch.unique(idx).numel() != n:
        raise ValueError('%s has a duplicate index: every output element must have one owner' % name)
    return idx.to(torch.int32).contiguous()


@torch.no_grad()
def psf_gram(geom, w, rs=None, cs=None, geom_q=None, out=None, rows=None, cols=None, accumulate=False):
    """
    out[f, rows[i], cols[j]] (= or +=) rs[f, i] cs[f, j] sum_b w[b, f] cos(2 pi nu_f / c (b_b . s_i - b_b . t_j)): the real
    part of A^T w conj(A) of the fringe matrix, without A (rime_psf_gram).  geom: the FringeGeometry of ONE time step whose
    first geom.P directions are the rows s_i (imaging.geometry); geom_q: another one over the same baselines and channels
    for the columns t_j, or None: the rows again (symmetric form, half the tiles computed, each stored twice).
    w (Nbl, Nf) or (Nbl, 1), real: its dtype is the working dtype.  rs (Nf, P) and cs (Nf, Pq), or None (1).  out
    (Nf, ldr, ldc), contiguous, of the working dtype, or None: a new (Nf, P, Pq); rows / cols: unique indices into its
    last two axes, or None (identity).  accumulate: add to out.  Deterministic (no atomics); no autograd.  Shapes, dtypes
    and index maps are checked first, the device last: every refusal comes before the launch.
    """
    dev = w.device
    if w.dtype not in (torch.float32, torch.float64):
        raise TypeError('psf_gram: w must be float32 or float64, got %s' % w.dtype)
    code, rdt = _real_dtype(w)
    Nbl, Nf = geom.Nbl, geom.Nf
    if geom.Nt != 1 or (geom_q is not None and geom_q.Nt != 1):
        raise ValueError('psf_gram takes geometries of one time step')
    if w.ndim != 2 or w.shape[0] != Nbl or w.shape[1] not in (1, Nf):
        raise ValueError('psf_gram: w must be (%d, %d) or (%d, 1), got %s' % (Nbl, Nf, Nbl, tuple(w.shape)))
    if any(s < 0 for s in w.stride()):
        w = w.contiguous()
    w_sb, w_sf = (w.stride(0) if Nbl > 1 else 0), (w.stride(1) if w.shape[1] > 1 else 0)
    Pr = int(getattr(geom, 'P', geom.Pstride))
    Pq = Pr
    if geom_q is not None:
        Pq = int(getattr(geom_q, 'P', geom_q.Pstride))
        same = lambda a, b: a.data_ptr() == b.data_ptr() and a.shape == b.shape or torch.equal(a, b)
        if geom_q.Nbl != Nbl or geom_q.Nf != Nf or not same(geom_q.blvecs, geom.blvecs) or not same(geom_q.freqs, geom.freqs):
            raise ValueError('psf_gram: geom_q must share blvecs and freqs with geom')
    if Pr <= 0 or Pq <= 0:
        raise ValueError('psf_gram: no pixels')
    scale = lambda x, P, name: None if x is None else _dense(torch.broadcast_to(x, (Nf, P)), rdt)
    rs, cs = scale(rs, Pr, 'rs'), scale(cs, Pq, 'cs')
    if out is None:
        if rows is not None or cols is not None or accumulate:
            raise ValueError('psf_gram: rows, cols and accumulate address an `out` the caller supplies')
        out = torch.empty(Nf, Pr, Pq, dtype=rdt, device=dev)
    if out.dtype != rdt:
        raise TypeError('psf_gram: out is %s, the working dtype (that of w) %s' % (out.dtype, rdt))
    if out.ndim != 3 or out.shape[0] != Nf or not out.is_contiguous():
        raise ValueError('psf_gram: out must be contiguous (%d, ldr, ldc), got %s' % (Nf, tuple(out.shape)))
    ldr, ldc = out.shape[1], out.shape[2]
    rows = _psf_index(rows, Pr, ldr, 'rows', dev)
    cols = _psf_index(cols, Pq, ldc, 'cols', dev)
    if (rows is None and ldr < Pr) or (cols is None and ldc < Pq):
        raise ValueError('psf_gram: out %s is smaller than the %d x %d pixels' % (tuple(out.shape), Pr, Pq))
    _require_cuda(geom.blvecs, geom.sdir, geom.freqs, w, rs, cs, out, geom_q.sdir if geom_q is not None else None)
    with _timed('psf_gram_kernel', Nbl * Nf * Pr * Pq):
        rc = lib.rime_psf_gram(code, _ptr(geom.blvecs), _ptr(geom.freqs), _ptr(w), w_sb, w_sf, Nbl, Nf,
                               _ptr(geom.sdir), geom.Pstride, Pr, _ptr(geom_q.sdir if geom_q is not None else None),
                               geom_q.Pstride if geom_q is not None else 0, Pq if geom_q is not None else 0,
                               _ptr(rs), _ptr(cs), _ptr(rows), _ptr(cols), _ptr(out), ldr, ldc, int(bool(accumulate)), _stream())
        check(rc, 'rime_psf_gram')
    return out


# ---------------------------------------------------------------------------------------
# log-priors on the fused prior kernel (csrc/prior.hip; DESIGN.md, "Log-priors")
# ---------------------------------------------------------------------------------------
PRIOR_KINDS = {'laplace': 0, 'taper_sigmoid': 1, 'taper_tanh': 2}
PRIOR_SIDES = {'both': 0, 'upper': 1, 'lower': 2}
PRIOR_OPERANDS = ('mean', 'scale', 'lower', 'upper', 'coeff')
PRIOR_THREADS, PRIOR_LANE_BYTES = 256, 32        # rime::PRIOR_THREADS, rime::PRIOR_BYTES: a chunk is their product in bytes
PRIOR_MAX_BLOCKS = lib.rime_prior_workspace() // 8      # one double per work-group: the grid's cap


def prior_grid_span(dtype):
    """elements of `dtype` that one full grid of the prior kernels covers: above it the grid-stride loop takes a second trip"""
    return PRIOR_MAX_BLOCKS * PRIOR_THREADS * PRIOR_LANE_BYTES // torch.empty((), dtype=dtype).element_size()


def _prior_period(shape, op):
    """the kernel's address mode of an operand against x of `shape`: 0 absent (None), 1 one value, N a full tensor, the
    product of the trailing axes it spans for a trailing broadcast; None for what the kernel does not serve"""
    if op is None:
        return 0
    if not torch.is_tensor(op):
        return 1 if isinstance(op, (int, float)) and not isinstance(op, bool) else None
    if op.is_complex() or not op.is_floating_point():
        return None
    if op.numel() == 1:
        return 1
    s = tuple(op.shape)
    while s and s[0] == 1:
        s = s[1:]
    if len(s) > len(shape) or tuple(shape[len(shape) - len(s):]) != s:
        return None
    return int(np.prod(s, dtype=np.int64))


def prior_fits(x, operands):
    """
    Whether prior_eval serves x with these operands (a sequence; None entries are absent operands): x a real float32 or
    float64 tensor on the GPU with at least one element, every operand a real number or real floating tensor that is one
    value, x's own shape, or the shape of trailing axes of x (leading axes of length 1 ignored).  Complex tensors, CPU
    tensors and broadcasts along a middle axis or beyond x's shape are refused: their callers compose the law in torch.
    """
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.numel() > 0):
        return False
    return all(_prior_period(x.shape, o) is not None for o in operands)


def _prior_fwd_call(kind, side, x, operands, out, dx):
    """rime_prior_fwd on a contiguous x with its five operands (PRIOR_OPERANDS order; dense tensors of x's dtype or None);
    dx None: no derivative is stored"""
    code, _ = _real_dtype(x)
    args = []
    for o in operands:
        args += [_ptr(o), 0 if o is None else _prior_period(x.shape, o)]
    ws, nws = _workspace(lib.rime_prior_workspace(), x.device)
    with _timed('prior_fwd_kernel', x.numel()):
        rc = lib.rime_prior_fwd(code, PRIOR_KINDS[kind], PRIOR_SIDES[side], _ptr(x), x.numel(), *args, _ptr(out), _ptr(dx),
                                _ptr(ws), nws, _stream())
        check(rc, 'rime_prior_fwd')


class _PriorEval(torch.autograd.Function):
    """sum of the prior's terms with the per-element derivative from the same pass; backward g dx (see rime_prior_fwd)"""
    @staticmethod
    def forward(ctx, x, kind, side, operands, keep):
        _require_cuda(x)
        xc = x.detach().contiguous()
        _, rdt = _real_dtype(xc)
        ops_ = [None if o is None else _dense(torch.as_tensor(o).to(xc.device), rdt) for o in operands]
        out = torch.empty((), dtype=rdt, device=xc.device)
        dx = torch.empty_like(xc) if keep else None
        _prior_fwd_call(kind, side, xc, ops_, out, dx)
        ctx.saved = dx
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dx = ctx.saved
        code, rdt = _real_dtype(dx)
        gx = torch.empty_like(dx)
        gg = g.detach().to(rdt).reshape(1).contiguous()
        rc = lib.rime_prior_bwd(code, _ptr(dx), _ptr(gg), dx.numel(), _ptr(gx), _stream())
        check(rc, 'rime_prior_bwd')
        return gx, None, None, None, None


def prior_eval(kind, x, mean=None, scale=None, lower=None, upper=None, coeff=None, side='both'):
    """
    The summed log-prior of a real GPU tensor x on the fused kernel, a 0-d tensor of x's dtype:
      'laplace'        sum -|r| / scale, r = x - mean; side 'upper' drops r < 0, 'lower' drops r > 0
      'taper_sigmoid'  sum logsig(coeff (x - lower)) + logsig(-coeff (x - upper)), logsig(z) = min(z, 0) - log1p(exp(-|z|))
      'taper_tanh'     sum log tanh(coeff (x - lower)) + log tanh(-coeff (x - upper)); NaN outside a bound
    lower or upper None drops its term.  The operands are constants, cast to x's dtype, in the shapes of prior_fits (the
    caller checks it; ValueError otherwise).  Differentiable w.r.t. x: the derivative is computed in the forward pass and kept
    only when x requires grad; the backward scales it by the upstream gradient.
    """
    operands = (mean, scale, lower, upper, coeff)
    if kind not in PRIOR_KINDS or side not in PRIOR_SIDES:
        raise ValueError('unknown prior kind %r or side %r' % (kind, side))
    if not prior_fits(x, operands):
        raise ValueError('prior_eval: x or an operand is not served by the fused kernel (see prior_fits)')
    keep = x.requires_grad and torch.is_grad_enabled()           # read here: grad mode is off inside forward
    return _PriorEval.apply(x, kind, side, operands, keep)


# ---------------------------------------------------------------------------------------
def _antenna_incidence(idx, Nant, dtype):
    """dense 0/1 [Nant, Nbl] matrix of which baselines an antenna slot takes part in (cached on idx)"""
    tag = getattr(idx, '_rime_incidence', None)
    if tag is not None and tag[0] == (idx._version, Nant, dtype):
        return tag[1]
    M = torch.zeros(Nant, idx.numel(), dtype=dtype, device=idx.device)
    M[idx.long(), torch.arange(idx.numel(), device=idx.device)] = 1
    try:
        idx._rime_incidence = ((idx._version, Nant, dtype), M)
    except Exception:
        pass
    return M


class _ApplyCal(torch.autograd.Function):
    """V' = G1 V G2^dagger in one pass over the visibilities; backward in one pass + two incidence products"""
    @staticmethod
    def forward(ctx, vis, gains, a1, a2, diag):
        _require_cuda(vis, gains, a1, a2)
        assert vis.is_complex() and gains.is_complex(), 'complex visibilities and gains'
        NP = vis.shape[0]
        assert vis.ndim == 5 and gains.ndim == 5 and vis.shape[:2] == (NP, NP) and gains.shape[:2] == (NP, NP)
        assert NP in (1, 2), 'Npol must be 1 or 2'
        _, _, Nbl, Nt, Nf = vis.shape
        Nant, Ntg, Nfg = gains.shape[2:]
        assert Ntg in (1, Nt) and Nfg in (1, Nf), 'gains must match or broadcast over time / channel'
        assert a1.dtype == torch.int32 and a2.dtype == torch.int32 and a1.numel() == Nbl and a2.numel() == Nbl
        v = vis.detach().contiguous()
        g = gains.detach().to(v.dtype).contiguous()
        code, _ = _real_dtype(v)
        st = (Nant * Ntg * Nfg, Ntg * Nfg, Nfg if Ntg > 1 else 0, 1 if Nfg > 1 else 0)
        out = torch.empty_like(v)
        rc = lib.rime_apply_cal_fwd(code, NP, int(bool(diag)), _ptr(torch.view_as_real(v)), _ptr(torch.view_as_real(g)),
                                    _ptr(a1), _ptr(a2), Nbl, Nt, Nf, Nant, *st, _ptr(torch.view_as_real(out)), _stream())
        check(rc, 'rime_apply_cal_fwd')
        ctx.saved = (v, g, a1, a2, st, bool(diag), gains.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        v, g, a1, a2, st, diag, gdt = ctx.saved
        NP, _, Nbl, Nt, Nf = v.shape
        Nant, Ntg, Nfg = g.shape[2:]
        code, rdt = _real_dtype(v)
        go = gout.detach().to(v.dtype).contiguous()
        gvis = torch.empty_like(v)
        d = torch.empty((2,) + tuple(v.shape), dtype=v.dtype, device=v.device)
        rc = lib.rime_apply_cal_bwd(code, NP, int(diag), _ptr(torch.view_as_real(v)), _ptr(torch.view_as_real(g)),
                                    _ptr(torch.view_as_real(go)), _ptr(a1), _ptr(a2), Nbl, Nt, Nf, Nant, *st,
                                    _ptr(torch.view_as_real(gvis)), _ptr(torch.view_as_real(d[0])),
                                    _ptr(torch.view_as_real(d[1])), _stream())
        check(rc, 'rime_apply_cal_bwd')
        ggains = None
        if ctx.needs_input_grad[1]:
            dr = torch.view_as_real(d).reshape(2, NP * NP, Nbl, Nt * Nf * 2)
            gg = torch.matmul(_antenna_incidence(a1, Nant, rdt), dr[0])
            gg += torch.matmul(_antenna_incidence(a2, Nant, rdt), dr[1])
            gg = torch.view_as_complex(gg.reshape(NP, NP, Nant, Nt, Nf, 2))
            if Ntg == 1 and Nt > 1:
                gg = gg.sum(3, keepdim=True)
            if Nfg == 1 and Nf > 1:
                gg = gg.sum(4, keepdim=True)
            ggains = gg.to(gdt)
        return (gvis if ctx.needs_input_grad[0] else None), ggains, None, None, None


def apply_cal(vis, gains, a1, a2, diag=False):
    """
    V'[p, q, b, t, f] = sum G1[p, r] V[r, s] conj(G2[q, s]) with G1 = gains[:, :, a1[b]], G2 = gains[:, :, a2[b]]
    (calibration._apply_cal, calibration.py:2412-2487, complex visibilities).  vis (Np, Np, Nbl, Nt, Nf)
    complex; gains (Np, Np, Nant, Nt | 1, Nf | 1) complex; a1, a2 int32 [Nbl] on the GPU.  diag: only the
    diagonal products, off-diagonal results zero (the reference's '2pol' mode).  Differentiable w.r.t.
    vis and gains.
    """
    return _ApplyCal.apply(vis, gains, a1, a2, diag)


# ---------------------------------------------------------------------------------------
ALM_SPLIT_F16 = True        # float32: f16 hi/lo split operands on the f16 matrix cores (22 bits) instead
                            # of the exact-f32 MFMA kernels (set False to force those)


def _ylm_scale(Y):
    """
    power of two bringing max|Ylm| to [2^10, 2^11].  Ylm matrices are reused every forward and a max
    over C3's 3 GB matrix costs as much as the transform itself, so the value is remembered ON the
    tensor object (with its version counter): a different tensor, or an in-place update, recomputes.
    """
    tag = getattr(Y, '_rime_yscale', None)
    if tag is not None and tag[0] == Y._version:
        return tag[1]
    amax = float(Y.detach().abs().amax().item())
    s = float(2.0 ** np.floor(np.log2(2048.0 / amax))) if amax > 0 and np.isfinite(amax) else 1.0
    try:
        Y._rime_yscale = (Y._version, s)
    except Exception:
        pass
    return s


ALM_PACKED = os.environ.get('RIME_ALM_PACKED', '1') != '0'      # cached pre-split f16 copies of Ylm in fragment order
ALM_PACKED_MIN_BYTES = 1 << 24                                   # below 16 MB of Ylm the transform is launch-bound anyway


# registry of the packed copies: id(Ylm tensor object) -> (weak reference to it, tag).  The copies are derived data that must
# not travel with the tensor (a torch.cuda.Event cannot be pickled or deep-copied, and a tensor's __dict__ is): a pickled /
# deep-copied model packs again on first use (round 5).  The weak reference's callback drops the entry -- and with it the two
# buffers -- when the tensor object dies; a recycled id() is caught by comparing the referent.
_YLM_PACKED = {}


def ylm_packed_state(Ylm):
    """the cache entry of this Ylm tensor OBJECT: (version, y_scale, data_ptr, {direction: (buffer, event, stream) | False}) or None"""
    ent = _YLM_PACKED.get(id(Ylm))
    return ent[1] if ent is not None and ent[0]() is Ylm else None


def _ylm_packed(Ylm, Y, ys, direction):
    """
    The packed copy of Ylm for one direction (0 forward, 1 backward; include/rime_hip.h: rime_alm2pix_pack), built on
    first use and remembered FOR the Ylm tensor object (module registry keyed on the object, see above) together with its
    version counter and y_scale -- a different tensor (AlmModel.setup_Ylm replaces it) or an in-place update packs again.
    Returns None when packing is switched
    off, the matrix is small, or the GPU has no room for another copy (the unpacked kernels then run).
    `Ylm` is the caller's tensor object (the cache belongs to it), `Y` its contiguous detached alias.

    MEMORY: each direction keeps a buffer of Ylm's own size on the device (8 bytes per (coefficient, pixel)): a model that
    runs forward AND backward holds THREE times the matrix (C3: 3.3 GB -> 9.9 GB) until the Ylm tensor is released or
    `release_ylm_packed(Ylm)` is called; RIME_ALM_PACKED=0 switches the copies off (kernels that split on the fly, ~25 %
    slower at the C3 shape).  A copy is only made while the device has that much free memory + 1 GB, counting the blocks the
    caching allocator holds but does not use; a refusal is re-examined on later calls (not remembered for the life of the
    tensor).  The pack kernel runs on the stream that is current at first use; an event recorded behind it is kept with
    the buffer, every later use on ANOTHER stream waits for it first and is recorded on the buffer (`record_stream`), so
    that releasing the copy while that stream still reads it cannot hand the block to a new owner.
    """
    if not ALM_PACKED or Y.dtype != torch.complex64 or ys <= 0 or Y.numel() * 8 < ALM_PACKED_MIN_BYTES:
        return None
    tag = ylm_packed_state(Ylm)
    if tag is None or tag[0] != Ylm._version or tag[1] != ys or tag[2] != Y.data_ptr():
        tag = (Ylm._version, ys, Y.data_ptr(), {})
        key = id(Ylm)
        try:
            import weakref
            _YLM_PACKED[key] = (weakref.ref(Ylm, lambda r, key=key: _YLM_PACKED.pop(key, None) if key in _YLM_PACKED and _YLM_PACKED[key][0] is r else None), tag)
        except TypeError:
            return None
    entry = tag[3].get(direction)
    stream = torch.cuda.current_stream(Y.device)
    if entry is None or entry is False:
        Nc, Npix = Y.shape
        nbytes = int(lib.rime_alm2pix_packed_bytes(Nc, Npix, direction))
        free, _ = torch.cuda.mem_get_info(Y.device)
        # blocks the caching allocator has reserved but not handed out are usable too
        free += torch.cuda.memory_reserved(Y.device) - torch.cuda.memory_allocated(Y.device)
        if nbytes == 0 or free < nbytes + (1 << 30):
            tag[3][direction] = False                    # no room NOW: asked again on the next call (two cheap queries)
            return None
        buf = torch.empty(nbytes, dtype=torch.uint8, device=Y.device)
        check(lib.rime_alm2pix_pack(_ptr(torch.view_as_real(Y)), ys, Nc, Npix, direction, _ptr(buf), _stream()), 'rime_alm2pix_pack')
        ready = torch.cuda.Event()
        ready.record(stream)
        entry = tag[3][direction] = (buf, ready, stream.cuda_stream)
    buf, ready, made_on = entry
    if made_on != stream.cuda_stream:
        stream.wait_event(ready)                         # packed on another stream: order this use behind the pack kernel
        buf.record_stream(stream)                        # ... and keep the block from being re-used under this stream's kernels
    return buf


def release_ylm_packed(Ylm):
    """drop the cached packed copies of `Ylm` (two buffers of its size; see _ylm_packed); they are rebuilt on the next use"""
    if ylm_packed_state(Ylm) is not None:
        _YLM_PACKED.pop(id(Ylm), None)


class _Alm2Pix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alm, Ylm):
        _require_cuda(alm, Ylm)
        assert alm.is_complex() and Ylm.is_complex()
        lead = alm.shape[:-1]
        Nc, Npix = Ylm.shape
        assert alm.shape[-1] == Nc
        a = alm.detach().contiguous()
        Y = Ylm.detach().contiguous()
        code, rdt = _real_dtype(a)
        assert Y.dtype == a.dtype, 'alm %s vs Ylm %s' % (a.dtype, Y.dtype)
        R = int(np.prod(lead)) if len(lead) else 1
        out = torch.empty(lead + (Npix,), dtype=rdt, device=a.device)
        ys = _ylm_scale(Ylm) if (rdt == torch.float32 and ALM_SPLIT_F16) else 0.0
        ws, nws = _workspace(lib.rime_alm2pix_fwd_workspace(code, R, Nc, Npix) if ys > 0 else 0, a.device, 16)
        packed = _ylm_packed(Ylm, Y, ys, 0) if ys > 0 else None
        if packed is not None:
            rc = lib.rime_alm2pix_fwd_packed(_ptr(torch.view_as_real(a)), _ptr(packed), ys, R, Nc, Npix, _ptr(out),
                                             _ptr(ws), nws, _stream())
            check(rc, 'rime_alm2pix_fwd_packed')
        else:
            rc = lib.rime_alm2pix_fwd(code, _ptr(torch.view_as_real(a)), _ptr(torch.view_as_real(Y)), ys,
                                      R, Nc, Npix, _ptr(out), _ptr(ws), nws, _stream())
            check(rc, 'rime_alm2pix_fwd')
        # the packed-copy cache lives on the CALLER's tensor object: a weak reference finds it again in the backward without
        # keeping that object (and its two packed buffers) alive through the graph
        import weakref
        ctx.Y, ctx.shape, ctx.dtype, ctx.ys, ctx.Ylm = Y, tuple(alm.shape), alm.dtype, ys, weakref.ref(Ylm)
        return out

    @staticmethod
    def backward(ctx, gout):
        Y = ctx.Y
        g = gout.contiguous()
        code, _ = _real_dtype(g)
        Nc, Npix = Y.shape
        ga = torch.empty(ctx.shape, dtype=ctx.dtype, device=g.device)
        R = int(np.prod(ctx.shape[:-1])) if len(ctx.shape) > 1 else 1
        ws, nws = _workspace(lib.rime_alm2pix_bwd_workspace(code, R, Nc, Npix), g.device, 16)
        owner = ctx.Ylm()
        packed = _ylm_packed(owner, Y, ctx.ys, 1) if (ctx.ys > 0 and owner is not None) else None
        if packed is not None:
            rc = lib.rime_alm2pix_bwd_packed(_ptr(g), _ptr(packed), ctx.ys, R, Nc, Npix,
                                             _ptr(torch.view_as_real(ga)), _ptr(ws), nws, _stream())
            check(rc, 'rime_alm2pix_bwd_packed')
        else:
            rc = lib.rime_alm2pix_bwd(code, _ptr(g), _ptr(torch.view_as_real(Y)), ctx.ys, R, Nc, Npix,
                                      _ptr(torch.view_as_real(ga)), _ptr(ws), nws, _stream())
            check(rc, 'rime_alm2pix_bwd')
        return ga, None


def alm2pix(alm, Ylm):
    """Re(alm @ Ylm): alm (..., Ncoeff) complex, Ylm (Ncoeff, Npix) complex -> (..., Npix) real."""
    return _Alm2Pix.apply(alm, Ylm)


# ---------------------------------------------------------------------------------------
# spherical Fourier-Bessel radial transform (csrc/sfb.hip)
SFB_TILE_ROWS, SFB_TILE_COLS = 64, 32        # rime::SFB_TI, rime::SFB_TC


class SFBPlan:
    """
    Device-side tables of one SFB radial transform (rime_sfb_fwd / _bwd): the real (Nk, Nr) matrices of all degrees packed
    into ONE buffer `g` (degree after degree in the order given, each row-major), int32 `blocks` [Nblk, 5] = (g_off, Nk,
    p_off, col_off, Nl), `cols` (the output columns of every degree), the forward tile list [(block, r0, c0)] over the
    (Nr x Nl) outputs and the backward one [(block, n0, c0)] over the (Nk x Nl) parameter blocks, and `covered`: whether
    every one of the Nlm output columns belongs to a degree (if not, the forward zero-fills its output first).
    mats: sequence of real 2-D (Nk, Nr) tensors / arrays (Nk may be 0); col_lists: their output columns.
    """
    def __init__(self, mats, col_lists, Nr, Nlm, dtype, device):
        assert dtype in (torch.float32, torch.float64), dtype
        # the device as tensors report it ('cuda' -> 'cuda:0'), so that it compares equal to params.device
        self.Nr, self.Nlm, self.dtype, self.device = int(Nr), int(Nlm), dtype, torch.empty(0, device=device).device
        blocks, cols, tf, tb, flat = [], [], [], [], []
        g_off = p_off = 0
        for bi, (G, cl) in enumerate(zip(mats, col_lists)):
            G = torch.as_tensor(G)
            if G.is_complex():
                raise ValueError('SFBPlan packs real matrices')
            if G.ndim != 2 or G.shape[1] != self.Nr:
                raise ValueError('degree %d: matrix of shape %s, expected (Nk, %d)' % (bi, tuple(G.shape), self.Nr))
            cl = np.asarray(cl, dtype=np.int64).ravel()
            if len(cl) and (cl.min() < 0 or cl.max() >= self.Nlm):
                raise ValueError('degree %d: output column outside [0, %d)' % (bi, self.Nlm))
            Nk, Nl = int(G.shape[0]), len(cl)
            blocks.append((g_off, Nk, p_off, len(cols), Nl))
            cols.extend(cl.tolist())
            flat.append(G.detach().to(device=self.device, dtype=dtype).reshape(-1))
            for c0 in range(0, Nl, SFB_TILE_COLS):
                tf.extend((bi, r0, c0) for r0 in range(0, self.Nr, SFB_TILE_ROWS))
                tb.extend((bi, n0, c0) for n0 in range(0, Nk, SFB_TILE_ROWS))
            g_off += Nk * self.Nr
            p_off += Nk * Nl
        if len(set(cols)) != len(cols):
            raise ValueError('two degrees claim the same output column')
        if max(g_off, p_off, self.Nr * self.Nlm) >= 2 ** 31:
            raise ValueError('SFB tables index with int32')
        self.Nlmn, self.Nblk = p_off, len(blocks)
        self.shapes = [(b[1], b[4]) for b in blocks]
        self.covered = len(cols) == self.Nlm
        i32 = lambda a, w: torch.as_tensor(np.asarray(a, dtype=np.int32).reshape(-1, w), device=self.device).contiguous()
        self.blocks, self.cols = i32(blocks, 5), i32(cols or [0], 1)      # never a null table
        self.tiles_fwd, self.tiles_bwd = i32(tf, 3), i32(tb, 3)
        self.g = torch.cat(flat) if flat else torch.zeros(0, dtype=dtype, device=self.device)
        if self.g.numel() == 0:
            self.g = torch.zeros(1, dtype=dtype, device=self.device)       # a valid pointer for the all-empty case


def _sfb_call(fn, name, inp, plan, tiles, cplx, B, res):
    with _timed(name.replace('rime_', '') + '_kernel', 2 * int(cplx + 1) * B * plan.Nr * plan.Nlmn):
        rc = fn(_dtype_code(plan.dtype), int(cplx), _ptr(inp), _ptr(plan.g), _ptr(plan.blocks), _ptr(plan.cols), _ptr(tiles),
                plan.Nblk, tiles.shape[0], B, plan.Nlmn, plan.Nr, plan.Nlm, _ptr(res), _stream())
        check(rc, name)


class _SFBRadial(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, plan):
        _require_cuda(params)
        p = params.detach().contiguous()
        _, rdt = _real_dtype(p)
        if rdt != plan.dtype or p.device != plan.device:
            raise TypeError('SFB plan built for %s on %s, parameters are %s on %s' % (plan.dtype, plan.device, p.dtype, p.device))
        if p.ndim < 1 or p.shape[-1] != plan.Nlmn:
            raise ValueError('parameters of shape %s, expected (..., %d)' % (tuple(p.shape), plan.Nlmn))
        batch = p.shape[:-1]
        B = int(np.prod(batch, dtype=np.int64))
        alloc = torch.empty if plan.covered else torch.zeros
        out = alloc(batch + (plan.Nr, plan.Nlm), dtype=p.dtype, device=p.device)
        _sfb_call(lib.rime_sfb_fwd, 'rime_sfb_fwd', p, plan, plan.tiles_fwd, p.is_complex(), B, out)
        ctx.plan, ctx.cplx, ctx.batch = plan, p.is_complex(), batch
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        plan = ctx.plan
        go = gout.detach().contiguous()
        B = int(np.prod(ctx.batch, dtype=np.int64))
        gp = torch.empty(ctx.batch + (plan.Nlmn,), dtype=go.dtype, device=go.device)
        _sfb_call(lib.rime_sfb_bwd, 'rime_sfb_bwd', go, plan, plan.tiles_bwd, ctx.cplx, B, gp)
        return gp, None


def sfb_radial(params, plan):
    """
    out[..., r, cols_l[c]] = sum_n g_l[n, r] params[..., p_off_l + n Nl + c] for every degree l of `plan` (an SFBPlan) in
    one launch; params (..., Nlmn) real or complex in the plan's precision -> (..., Nr, Nlm) of the same dtype, columns
    without a degree 0.  Differentiable w.r.t. params (one launch); the basis is fixed.
    """
    return _SFBRadial.apply(params, plan)


# ---------------------------------------------------------------------------------------
# grouped matrix filter along the last axis (csrc/filt.hip)
FILT_TILE_LINES, FILT_TILE_ROWS = 64, 128    # rime::FILT_TL, rime::FILT_TC


def filt_pack(W):
    """
    Filters [Nfilt, R, C] (real or complex) as the real, contraction-major buffer rime_filt_apply reads: [Nfilt, C, R] for a
    real W; [Nfilt, 2C, R] for a complex one, rows 2c / 2c + 1 holding Re W[:, :, c] / -Im W[:, :, c].
    """
    W = torch.as_tensor(W)
    if W.ndim != 3:
        raise ValueError('filters of shape %s, expected (Nfilt, rows, columns)' % (tuple(W.shape),))
    if W.is_complex():
        Nf, R, C = W.shape
        return torch.view_as_real(W.conj().resolve_conj()).reshape(Nf, R, 2 * C).transpose(1, 2).contiguous()
    return W.transpose(1, 2).contiguous()


def filt_tables(M, K, residual=False, input_idx=None):
    """
    The index tables of both directions of y = filter(x) with a (M, K) matrix G (numpy; see rime_filt_apply):
    a dict with 'fwd' and 'bwd', each (ic int32, oc int32, base float64, s), and 'Ny', the length of an output line.
    input_idx: None, or the M columns of the input (integers or a boolean mask of length K) the filtered samples replace.
    """
    M, K = int(M), int(K)
    idx = None
    if input_idx is not None:
        idx = _host_array(input_idx)
        if idx.dtype == bool:
            if idx.shape != (K,):
                raise ValueError('boolean input_idx of shape %s, the filtered axis has %d samples' % (idx.shape, K))
            idx = np.nonzero(idx)[0]
        idx = idx.astype(np.int64).ravel()
        idx = np.where(idx < 0, idx + K, idx)
        if len(idx) != M:
            raise ValueError('input_idx selects %d samples, G has %d rows' % (len(idx), M))
        if len(idx) and (idx.min() < 0 or idx.max() >= K):
            raise ValueError('input_idx outside [0, %d)' % K)
        if len(np.unique(idx)) != len(idx):
            raise ValueError('input_idx repeats a sample')
    elif residual and M != K:
        raise ValueError('residual of a (%d, %d) filter: the output has another length than the input' % (M, K))
    s = -1.0 if residual else 1.0
    eyeK, eyeM = np.arange(K, dtype=np.int32), np.arange(M, dtype=np.int32)
    sel = eyeM if idx is None else idx.astype(np.int32)
    fwd = (eyeK, sel, np.full(M, 1.0 if residual else 0.0), s)
    if residual:
        bbase = np.ones(K)
    elif idx is None:
        bbase = np.zeros(K)
    else:
        bbase = np.ones(K)
        bbase[idx] = 0.0
    bwd = (sel, eyeK, bbase, s)
    return {'fwd': fwd, 'bwd': bwd, 'Ny': M if idx is None else K, 'idx': idx}


def filt_tiles(outer, Nbl, inner, bl2filt, with_pass=True):
    """
    Tile list of a tensor of outer x Nbl x inner lines (line = (o Nbl + b) inner + t) whose baseline b uses filter
    bl2filt[b] (-1: none): int32 [Ntile, 65] = (filter, 64 line indices).  Lines are grouped by filter, filters ascending,
    lines ascending inside a filter, -1 padding only at the end of a filter's last tile; the tiles of the unfiltered lines
    (filter -1) come last and are left out when with_pass is False.  Returns (tiles, number of pass-through tiles).
    """
    b2f = np.asarray(bl2filt, dtype=np.int64).ravel()
    if len(b2f) != Nbl:
        raise ValueError('%d filter indices for %d baselines' % (len(b2f), Nbl))
    if outer * Nbl * inner >= 2 ** 31:
        raise ValueError('filter tables index lines with int32')
    fl = np.broadcast_to(b2f[None, :, None], (outer, Nbl, inner)).reshape(-1)
    out, npass = [], 0
    order = sorted(f for f in np.unique(b2f) if f >= 0) + ([-1] if (with_pass and (b2f < 0).any()) else [])
    for f in order:
        lines = np.nonzero(fl == f)[0] if f >= 0 else np.nonzero(fl < 0)[0]
        nt = -(-len(lines) // FILT_TILE_LINES)
        padded = np.full(nt * FILT_TILE_LINES, -1, dtype=np.int32)
        padded[:len(lines)] = lines
        t = np.empty((nt, 1 + FILT_TILE_LINES), dtype=np.int32)
        t[:, 0] = f
        t[:, 1:] = padded.reshape(nt, FILT_TILE_LINES)
        out.append(t)
        if f < 0:
            npass = nt
    tiles = np.concatenate(out) if out else np.zeros((0, 1 + FILT_TILE_LINES), dtype=np.int32)
    return tiles, npass


class FiltPlan:
    """
    Device-side state of one grouped filter (rime_filt_apply) in one precision on one device: the filters G [Nfilt, M, K]
    (or [M, K]) packed for the forward (W = G) and the adjoint (W = G^H), the tables ic / oc / base of both directions
    (filt_tables) and the tile lists, cached per (outer, Nbl, inner, baseline -> filter, with_pass) layout.
    """
    def __init__(self, G, residual=False, input_idx=None, dtype=torch.float32, device='cuda'):
        assert dtype in (torch.float32, torch.float64), dtype
        G = torch.as_tensor(G)
        if G.requires_grad:
            raise ValueError('the filter matrix G requires grad: filt_apply differentiates with respect to the data only')
        if G.ndim == 2:
            G = G[None]
        if G.ndim != 3 or 0 in G.shape:
            raise ValueError('G of shape %s, expected (Nfilt, M, K) or (M, K)' % (tuple(G.shape),))
        self.dtype, self.device = dtype, torch.empty(0, device=device).device
        _require_cuda(torch.empty(0, device=self.device))
        self.Nfilt, self.M, self.K = (int(n) for n in G.shape)
        self.cplx, self.residual = G.is_complex(), bool(residual)
        tab = filt_tables(self.M, self.K, residual, input_idx)
        self.Ny, self.has_idx = tab['Ny'], tab['idx'] is not None
        G = G.detach().to(device=self.device, dtype=(_lib_cdtype(dtype) if self.cplx else dtype))
        dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), device=self.device).to(dt).contiguous()
        self.W = {'fwd': filt_pack(G), 'bwd': filt_pack(G.transpose(1, 2).conj() if self.cplx else G.transpose(1, 2))}
        self.tab = {d: (dev(tab[d][0], torch.int32), dev(tab[d][1], torch.int32), dev(tab[d][2], dtype), tab[d][3])
                    for d in ('fwd', 'bwd')}
        self._tiles = {}

    def tiles(self, outer, Nbl, inner, bl2filt, with_pass):
        key = (int(outer), int(Nbl), int(inner), tuple(int(f) for f in bl2filt), bool(with_pass))
        if key not in self._tiles:
            t, npass = filt_tiles(key[0], key[1], key[2], key[3], key[4])
            if len(t) and t[:, 0].max() >= self.Nfilt:
                raise ValueError('a baseline names filter %d, the plan holds %d' % (t[:, 0].max(), self.Nfilt))
            self._tiles[key] = (torch.as_tensor(t, device=self.device).contiguous(), npass)
        return self._tiles[key]


def _lib_cdtype(dtype):
    return torch.complex64 if dtype == torch.float32 else torch.complex128


def _filt_call(plan, direction, x, y, tiles, npass):
    ic, oc, base, s = plan.tab[direction]
    M, K = (plan.M, plan.K) if direction == 'fwd' else (plan.K, plan.M)
    Nx, Ny = x.shape[-1], y.shape[-1]
    nlines = x.numel() // Nx
    with _timed('filt_kernel', 2 * (4 if plan.cplx else 2) * nlines * M * K):
        rc = lib.rime_filt_apply(_dtype_code(plan.dtype), int(plan.cplx), _ptr(x), _ptr(plan.W[direction]),
                                 _ptr(ic), _ptr(oc), _ptr(base), _ptr(tiles), tiles.shape[0], npass, plan.Nfilt, M, K, Nx, Ny,
                                 nlines, s, _ptr(y), _stream())
        check(rc, 'rime_filt_apply')


class _FiltApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan, layout):
        _require_cuda(x)
        xc = x.detach().contiguous()
        if not xc.is_complex():
            raise TypeError('filt_apply runs on complex lines, got %s' % xc.dtype)
        _, rdt = _real_dtype(xc)
        if rdt != plan.dtype or xc.device != plan.device:
            raise TypeError('filter plan built for %s on %s, data are %s on %s' % (plan.dtype, plan.device, xc.dtype, xc.device))
        if xc.ndim < 1 or xc.shape[-1] != plan.K:
            raise ValueError('data of shape %s, the filter takes %d samples along the last axis' % (tuple(xc.shape), plan.K))
        batch = xc.shape[:-1]
        nlines = int(np.prod(batch, dtype=np.int64))
        if layout is None:
            layout = (1, 1, (0,))
        Nbl, inner, b2f = layout
        if Nbl * inner == 0 or nlines % (Nbl * inner):
            raise ValueError('%d lines do not divide into %d baselines x %d' % (nlines, Nbl, inner))
        outer = nlines // (Nbl * inner)
        if min(b2f) < 0 and plan.Ny != plan.K:
            raise ValueError('unfiltered baselines pass through unchanged, but the filter maps %d samples to %d' % (plan.K, plan.Ny))
        if plan.has_idx:
            y = xc.clone()                              # the kernel writes the input_idx columns of the filtered lines only
        else:
            y = torch.empty(batch + (plan.Ny,), dtype=xc.dtype, device=xc.device)
        if nlines:
            tiles, npass = plan.tiles(outer, Nbl, inner, b2f, not plan.has_idx)
            _filt_call(plan, 'fwd', xc, y, tiles, npass)
        ctx.plan, ctx.geom = plan, (outer, Nbl, inner, b2f)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        plan = ctx.plan
        g = gy.detach().contiguous()
        gx = torch.empty(g.shape[:-1] + (plan.K,), dtype=g.dtype, device=g.device)
        if gx.numel():
            tiles, npass = plan.tiles(*ctx.geom, True)
            _filt_call(plan, 'bwd', g, gx, tiles, npass)
        return gx, None, None


def filt_apply(x, plan, dim=-1, layout=None):
    """
    y[l, oc[i]] = s sum_k G[f(l)][i, k] x[l, k] + base[i] x[l, oc[i]] along axis `dim` of a complex x, in one launch
    (rime_filt_apply) and one more backwards; `plan` is a FiltPlan.  layout = (Nbl, inner, bl2filt): the lines of x (all axes
    but `dim`, flattened) are outer x Nbl x inner and baseline b uses filter bl2filt[b], -1 leaving its lines as they are;
    None: every line uses filter 0.  Only the last, contiguous axis runs in the kernel: any other `dim` costs one extra
    transposition pass each way (movedim(dim, -1).contiguous(), kernel, movedim back), and `layout` then describes the lines
    of the transposed tensor.  A real x is filtered as a complex one with a zero imaginary part (one more pass) and comes
    back real when G is real.  Differentiable with respect to x only.
    """
    _require_cuda(x)
    if x.ndim < 1:
        raise ValueError('filt_apply needs at least one axis')
    if layout is not None:
        layout = (int(layout[0]), int(layout[1]), tuple(int(f) for f in layout[2]))
    was_real = not x.is_complex()
    if was_real:
        x = torch.complex(x, torch.zeros_like(x))
    d = dim % x.ndim
    if d != x.ndim - 1:
        x = x.movedim(d, -1)
    y = _FiltApply.apply(x, plan, layout)
    if d != y.ndim - 1:
        y = y.movedim(-1, d)
    if was_real and not plan.cplx:
        y = y.real
    return y


# ---------------------------------------------------------------------------------------
# batched 1-D DFT along the last axis with window, shifts, norm and epilogue fused (csrc/fft.hip)
# ---------------------------------------------------------------------------------------
FFT_MAX_N = 4096
FFT_ABS, FFT_PEAKNORM, FFT_SQUARE, FFT_PEAK = 1, 2, 4, 8
_FFT_EPILOGUES = {'none': 0, 'abs': FFT_ABS, 'peaknorm': FFT_PEAKNORM, 'square': FFT_SQUARE, 'peak': FFT_PEAK}


def fft_radices(N):
    """
    Radix list of the Stockham passes of an N-point transform (product N): 4 while two factors of 2 are left, then a lone 2,
    then 3s, 5s and every other prime factor ascending (those run as generic p-term butterflies).  N = 1: no pass.
    """
    N = int(N)
    if N < 1:
        raise ValueError('transform length %d' % N)
    out, n = [], N
    while n % 4 == 0:
        out.append(4)
        n //= 4
    p = 2
    while n > 1:
        if p * p > n:
            p = n
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1 if p == 2 else 2
    return out


def fft_twiddles(N, inverse=False):
    """exp(-+2 pi i j / N), j < N (plus for inverse), numpy complex128: the table of rime_fft_apply before its one rounding"""
    return np.exp((2j if inverse else -2j) * np.pi * np.arange(int(N)) / int(N))


def fft_epilogue_mask(epilogue):
    """'none', 'abs', 'peaknorm', 'square', 'peak' or several joined by '+' -> the bit mask of rime_fft_apply; the kernel
    applies them in the reference's order abs -> peaknorm -> square (-> peak) whatever the order of the names"""
    if isinstance(epilogue, (int, np.integer)):
        mask = int(epilogue)
        if not 0 <= mask <= 15:
            raise ValueError('unknown fft epilogue %r' % (epilogue,))
        return mask
    mask = 0
    for name in str(epilogue).split('+'):
        if name not in _FFT_EPILOGUES:
            raise ValueError('unknown fft epilogue %r' % (epilogue,))
        mask |= _FFT_EPILOGUES[name]
    return mask


def fft_scale(N, inverse, norm):
    """the factor torch.fft applies: 'backward' (None) scales the inverse by 1/N, 'forward' the forward, 'ortho' both by 1/sqrt(N)"""
    if norm in (None, 'backward'):
        return 1.0 / N if inverse else 1.0
    if norm == 'forward':
        return 1.0 if inverse else 1.0 / N
    if norm == 'ortho':
        return 1.0 / np.sqrt(N)
    raise ValueError("norm %r, expected None, 'backward', 'forward' or 'ortho'" % (norm,))


class FFTPlan:
    """
    Host plan of an N-point transform in one precision on one device: the radix list and both twiddle tables
    exp(-+2 pi i j / N), computed in float64, rounded once to the precision of the run and kept on the device.  The tables
    are built on first use and dropped on pickling.
    """
    def __init__(self, N, dtype=torch.float32, device='cuda'):
        dtype = {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(dtype, dtype)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError('fft plan in %s: float32 or float64' % dtype)
        N = int(N)
        if N < 1 or N > FFT_MAX_N:
            raise ValueError('transform length %d: the kernel serves 1 ... %d' % (N, FFT_MAX_N))
        self.N, self.dtype, self.device = N, dtype, torch.device(device)
        self.radix = fft_radices(N)
        self._radix_c = (ctypes.c_int * max(1, len(self.radix)))(*self.radix)

    def table(self, inverse, device=None):
        device = self.device if device is None else torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError("bayeslim_amd ops need tensors on the GPU (got device '%s'); there is no CPU implementation" % device)
        tw = self.__dict__.setdefault('_tw', {})
        key = (bool(inverse), str(device))
        if key not in tw:
            tw[key] = torch.as_tensor(fft_twiddles(self.N, key[0])).to(_lib_cdtype(self.dtype)).to(device).contiguous()
        return tw[key]

    def serves(self, device):
        """whether the plan's device names `device` ('cuda' without an index names every GPU)"""
        return device.type == self.device.type and self.device.index in (None, device.index)

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_tw', None)
        state.pop('_radix_c', None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._radix_c = (ctypes.c_int * max(1, len(self.radix)))(*self.radix)


def _fft_call(plan, x, inverse, sh_in, sh_out, window, win_store, scale, mask, start, df):
    """one launch of rime_fft_apply on the lines of a contiguous complex x [..., N]"""
    N = plan.N
    batch = tuple(x.shape[:-1])
    nlines = int(np.prod(batch, dtype=np.int64))
    rdt = plan.dtype
    if mask & FFT_PEAK:
        y = torch.empty(batch + (1,), dtype=rdt, device=x.device)
    elif mask & (FFT_ABS | FFT_SQUARE):
        y = torch.empty(batch + (N,), dtype=rdt, device=x.device)
    else:
        y = torch.empty(batch + (N,), dtype=x.dtype, device=x.device)
    if nlines == 0:
        return y
    with _timed('fft_kernel', nlines * N):
        rc = lib.rime_fft_apply(_dtype_code(rdt), _ptr(x), _ptr(plan.table(inverse, x.device)), _ptr(window),
                                int(win_store), plan._radix_c, len(plan.radix), N, nlines, int(bool(inverse)), int(sh_in), int(sh_out),
                                float(scale), int(mask), float(start), float(df), _ptr(y), _stream())
        check(rc, 'rime_fft_apply')
    return y


class _FFTApply(torch.autograd.Function):
    """the linear part y = P_out s F P_in W x and its adjoint W P_in^H s F^H P_out^H through the same kernel"""
    @staticmethod
    def forward(ctx, x, plan, inverse, sh_in, sh_out, window, scale, mask, start, df):
        xc = x.detach().contiguous()
        y = _fft_call(plan, xc, inverse, sh_in, sh_out, window, False, scale, mask, start, df)
        ctx.plan, ctx.args, ctx.window = plan, (inverse, sh_in, sh_out, scale), window
        if mask:
            ctx.mark_non_differentiable(y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        plan, N = ctx.plan, ctx.plan.N
        inverse, sh_in, sh_out, scale = ctx.args
        g = gy.detach().contiguous()
        gx = _fft_call(plan, g, not inverse, (N - sh_out) % N, (N - sh_in) % N, ctx.window, True, scale, 0, 0.0, 1.0)
        return (gx,) + (None,) * 9


def fft_apply(x, plan, dim=-1, inverse=False, window=None, shift=False, norm=None, epilogue='none', start=0.0, df=1.0):
    """
    The reference's FFT block along axis `dim` of x in one launch of rime_fft_apply (`plan` an FFTPlan of that length):
    multiply by the real `window` (a vector of N samples, or None), ifftshift (inverse and shift), transform (`inverse`:
    the ifft), scale as torch.fft does for `norm`, fftshift (forward and shift), then the epilogue: 'none' (complex out),
    'abs', 'square' (|.|^2), 'peaknorm' (divide the line by its max |.|), or several joined by '+', applied in the
    reference's order abs -> peaknorm -> square.  With 'peak' (alone or after the others) the result is one real per line,
    length 1 along `dim`: start + (n + delta) df with n the first index of the line's maximum and delta Quinn's second
    estimator from the neighbours of n (wrapping round); not differentiable.

    Differentiable with respect to x through the linear part (one more launch: conjugate twiddles, window on the store,
    shifts swapped, the same scale); no gradient flows to the window.  The non-linear epilogues are fused only when no
    gradient is asked for (torch.no_grad(), or x does not require grad); otherwise the kernel returns the complex
    spectrum and abs / peak normalisation / square are the reference's torch expressions.  Only the last, contiguous axis
    runs in the kernel: any other `dim` costs movedim(dim, -1).contiguous() and a movedim back.  A real x is promoted to
    complex first.
    """
    _require_cuda(x)
    if x.ndim < 1:
        raise ValueError('fft_apply needs at least one axis')
    if not x.is_complex():
        if not x.is_floating_point():
            x = x.to(plan.dtype)
        x = torch.complex(x, torch.zeros_like(x))
    _, rdt = _real_dtype(x)
    if rdt != plan.dtype or not plan.serves(x.device):
        raise TypeError('fft plan built for %s on %s, data are %s on %s' % (plan.dtype, plan.device, x.dtype, x.device))
    d = dim % x.ndim
    if d != x.ndim - 1:
        x = x.movedim(d, -1)
    N = plan.N
    if x.shape[-1] != N:
        raise ValueError('data of shape %s along the transformed axis last, the plan transforms %d samples' % (tuple(x.shape), N))
    if window is not None:
        window = torch.as_tensor(window).detach()
        if window.is_complex() or window.numel() != N:
            raise ValueError('the window is a real vector of %d samples' % N)
        window = window.reshape(N).to(device=x.device, dtype=rdt).contiguous()
    mask = fft_epilogue_mask(epilogue)
    scale = fft_scale(N, inverse, norm)
    sh_in = N // 2 if (shift and inverse) else 0
    sh_out = (N - N // 2) % N if (shift and not inverse) else 0
    needs_grad = torch.is_grad_enabled() and x.requires_grad
    if mask & FFT_PEAK:
        x, needs_grad = x.detach(), False
    if mask == 0 or not needs_grad:
        y = _FFTApply.apply(x, plan, bool(inverse), sh_in, sh_out, window, scale, mask, start, df)
    else:
        y = _FFTApply.apply(x, plan, bool(inverse), sh_in, sh_out, window, scale, 0, 0.0, 1.0)
        if mask & FFT_ABS:
            y = torch.abs(y)
        if mask & FFT_PEAKNORM:
            y = y / torch.max(torch.abs(y), dim=-1, keepdim=True).values
        if mask & FFT_SQUARE:
            y = torch.abs(y) ** 2
    if d != y.ndim - 1:
        y = y.movedim(-1, d)
    return y


# ---------------------------------------------------------------------------------------
# linear model y = A x along any axis with gather, coeff and real part fused (csrc/lm.hip)
# ---------------------------------------------------------------------------------------
LM_REG = 32          # rime::LM_REG: the register limit between the few-in and the few-out form of the strided kernels


def lm_layout(R, K, I):
    """
    The storage order of M [R, K] for one launch: 'rk' (row-major, k contiguous) for the few-in strided kernels (I > 1,
    K <= 32), which read a row of M per output row; 'kr' (r contiguous) for the few-out strided kernels and for the last-axis
    kernel (I == 1), which read a column of M per input.
    """
    return 'rk' if (I > 1 and K <= LM_REG) else 'kr'


class LMPlan(_IndexPlan):
    """
    Device-side state of one linear model y = A x (rime_lm_apply): the design matrix A (Nsamples, Nfeatures), real or complex,
    the gather table idx along the contracted axis and the vector coeff of the un-gathered axis (or None).  The tables the
    kernel reads -- A for the forward, A^H for the adjoint, each also as its real part and in either storage order
    (lm_layout) -- are built on first use per precision and device from the master copy, which is kept as given, and dropped
    on pickling and deep copies; a rebuilt table holds the same bits.  pre = coeff[idx] scales the gathered inputs.
    """
    def __init__(self, A, idx=None, coeff=None):
        A = torch.as_tensor(A)
        if A.requires_grad:
            raise ValueError('the design matrix A requires grad: lm_apply differentiates with respect to the input only')
        if A.ndim == 1:
            A = A[:, None]                                 # one feature
        if A.ndim != 2 or 0 in A.shape:
            raise ValueError('A of shape %s, expected (Nsamples, Nfeatures)' % (tuple(A.shape),))
        if not (A.is_floating_point() or A.is_complex()):
            A = A.to(torch.get_default_dtype())
        self.A = A.detach()
        self.R, self.K = (int(n) for n in A.shape)
        self.cplx = A.is_complex()
        self.idx = self.coeff = None
        self.K_in = None
        if coeff is not None:
            coeff = torch.as_tensor(coeff).detach().reshape(-1)
            if coeff.is_complex():
                raise TypeError('the fused coeff is a real vector; multiply a complex one into the input first')
            self.coeff, self.K_in = coeff, int(coeff.numel())
        if idx is not None:
            idx = torch.as_tensor(idx).detach().reshape(-1).to(torch.int64)
            if idx.numel() != self.K:
                raise ValueError('idx names %d entries, A takes %d features' % (idx.numel(), self.K))
            self.idx = idx
            self.idx_min, self.idx_max = int(idx.min()), int(idx.max())
            if self.idx_min < 0 or (self.K_in is not None and self.idx_max >= self.K_in):
                raise IndexError('idx outside the indexed axis')
        elif self.K_in is not None and self.K_in != self.K:
            raise ValueError('coeff of %d entries, A takes %d features' % (self.K_in, self.K))

    def table(self, direction, real_part, layout, dtype, device):
        """(buffer, m_rs, m_ks, R, K, complex) of M = A ('fwd') or A^H ('bwd'), or of Re(M), stored in `layout`"""
        device = torch.device(device)
        key = ('M', direction, bool(real_part), layout, dtype, str(device))
        tabs = self._cache()
        if key not in tabs:
            M = self.A.to(device=device, dtype=(_lib_cdtype(dtype) if self.cplx else dtype))
            if direction == 'bwd':
                M = M.conj().T if self.cplx else M.T
            if real_part and self.cplx:
                M = M.real
            R, K = (int(n) for n in M.shape)
            if layout == 'rk':
                buf, rs, ks = M.resolve_conj().contiguous(), K, 1
            else:
                buf, rs, ks = M.T.resolve_conj().contiguous(), 1, R
            tabs[key] = (buf, rs, ks, R, K, buf.is_complex())
        return tabs[key]

    def matrix(self, direction, real_part, layout, dtype, device):
        """the table as the matrix the kernel multiplies with, [R, K] (a view of the buffer)"""
        buf, rs, ks, R, K, _ = self.table(direction, real_part, layout, dtype, device)
        return buf if layout == 'rk' else buf.T

    def gather(self, device, dtype=torch.int32):
        """idx on the device, cached: int32 is the kernel's table, int64 what index_add_ / indexing take; None without idx"""
        if self.idx is None:
            return None
        key = ('idx', dtype, str(torch.device(device)))
        tabs = self._cache()
        if key not in tabs:
            tabs[key] = self.idx.to(device=device, dtype=dtype).contiguous()
        return tabs[key]

    def scale(self, dtype, device):
        """pre = coeff[idx] (coeff without idx) in the run's precision, or None"""
        if self.coeff is None:
            return None
        key = ('pre', dtype, str(torch.device(device)))
        tabs = self._cache()
        if key not in tabs:
            c = self.coeff.to(device=device, dtype=dtype)
            if self.idx is not None:
                c = c[self.gather(device, torch.int64)]
            tabs[key] = c.contiguous()
        return tabs[key]

    def __deepcopy__(self, memo):
        new = type(self).__new__(type(self))
        import copy
        new.__dict__.update({k: copy.deepcopy(v, memo) for k, v in self.__getstate__().items()})
        return new


def _lm_call(plan, direction, x3, real_out, with_idx=True):
    """
    one launch of rime_lm_apply on a contiguous x3 [O, K_in, I]: 'fwd' gathers through plan.idx, scales by pre and applies A;
    'bwd' applies A^H and scales the compact result [O, K, I] by pre.  real_out: Re(.) only.
    """
    O, K_in, I = (int(n) for n in x3.shape)
    code, rdt = _real_dtype(x3)
    xc = x3.is_complex()
    real_part = bool(real_out and not xc)                     # Re(M x) of a real x: Re(M) x
    R, K = (plan.R, plan.K) if direction == 'fwd' else (plan.K, plan.R)
    buf, rs, ks, R, K, mc = plan.table(direction, real_part, lm_layout(R, K, I), rdt, x3.device)
    idx = pre = post = None
    if direction == 'fwd':
        pre = plan.scale(rdt, x3.device)
        if with_idx:
            idx = plan.gather(x3.device)
        if idx is not None:
            if plan.idx_max >= K_in:
                raise IndexError('idx reaches entry %d, the indexed axis holds %d' % (plan.idx_max, K_in))
        elif K_in != K:
            raise ValueError('the contracted axis holds %d entries, A takes %d' % (K_in, K))
    else:
        post = plan.scale(rdt, x3.device)
        if K_in != K:
            raise ValueError('the contracted axis holds %d entries, A gives %d' % (K_in, K))
    out_real = bool(real_out and xc)
    ycplx = (xc or mc) and not out_real
    y = torch.empty((O, R, I), dtype=_lib_cdtype(rdt) if ycplx else rdt, device=x3.device)
    if y.numel() == 0:
        return y
    with _timed('lm_kernel', O * R * I * K):
        rc = lib.rime_lm_apply(code, int(xc), int(mc), int(out_real), _ptr(x3), _ptr(buf),
                               rs, ks, _ptr(idx), _ptr(pre), _ptr(post), O, K, K_in, R, I, _ptr(y), _stream())
        check(rc, 'rime_lm_apply')
    return y


def _lm_adjoint(plan, g3, K_in, want_real):
    """A^H g with the scaling, scattered through idx to [O, K_in, I]; real when want_real"""
    gx = _lm_call(plan, 'bwd', g3, want_real)
    if plan.idx is not None:
        full = torch.zeros((gx.shape[0], K_in, gx.shape[2]), dtype=gx.dtype, device=gx.device)
        gx = full.index_add_(1, plan.gather(gx.device, torch.int64), gx)
    return gx


class _LMApply(torch.autograd.Function):
    """y = A (coeff x)[idx] ('fwd') or its adjoint ('bwd') on x3 [O, K_in, I]; the backward pass is the other direction"""
    @staticmethod
    def forward(ctx, x3, plan, direction, out_real, K_in):
        xc = x3.detach().contiguous()
        ctx.plan, ctx.direction, ctx.xcplx, ctx.K_in, ctx.xdtype = plan, direction, xc.is_complex(), int(xc.shape[1]), xc.dtype
        if direction == 'fwd':
            return _lm_call(plan, 'fwd', xc, out_real)
        return _lm_adjoint(plan, xc, K_in, out_real)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        g = gy.detach().contiguous()
        if ctx.direction == 'fwd':
            gx = _lm_adjoint(ctx.plan, g, ctx.K_in, not ctx.xcplx)
        else:
            gx = _lm_call(ctx.plan, 'fwd', g, not ctx.xcplx)
        if gx.dtype != ctx.xdtype:
            gx = gx.to(ctx.xdtype)                            # a real product for a complex input: zero imaginary part
        return gx, None, None, None, None


def lm_apply(x, plan, dim=0, out_real=False, adjoint=False, K_in=None):
    """
    y = A (coeff * x)[idx] along axis `dim` of x in one launch of rime_lm_apply (`plan` an LMPlan): x of up to 8 axes maps onto
    [O, K_in, I] (the axes before `dim`, `dim`, the axes after it; the last axis, or a 1-D x, gives I = 1 and the last-axis
    kernel), and y has A's Nsamples entries along `dim`.  x and A are real or complex, y is complex when either is; with
    out_real only Re(A x) is computed and returned.  The run's precision is the wider of x's and A's.
    adjoint=True applies coeff[idx] * (A^H x) instead and scatters it through idx with index_add_ onto K_in entries (default:
    what the plan's coeff fixes, else A's Nfeatures).
    Differentiable once with respect to x only (the other direction through the same kernel; the scatter through idx is a torch
    index_add_); A, idx and coeff carry no gradient.  A non-contiguous x is made contiguous.  No CPU path.
    """
    _require_cuda(x)
    if x.ndim < 1 or x.ndim > 8:
        raise ValueError('lm_apply takes 1 to 8 axes, got %d' % x.ndim)
    if not (x.is_floating_point() or x.is_complex()):
        x = x.to(plan.A.real.dtype if plan.cplx else plan.A.dtype)
    rx, ra = _real_dtype(x)[1], _real_dtype(plan.A)[1]
    if rx != ra and ra == torch.float64:
        x = x.to(torch.complex128 if x.is_complex() else torch.float64)
    d = dim % x.ndim
    shape = tuple(x.shape)
    O, I = int(np.prod(shape[:d], dtype=np.int64)), int(np.prod(shape[d + 1:], dtype=np.int64))
    if adjoint:
        if K_in is None:
            K_in = plan.K_in if plan.K_in is not None else plan.K
        if plan.idx is not None and plan.idx_max >= K_in:
            raise IndexError('idx reaches entry %d, the indexed axis holds %d' % (plan.idx_max, K_in))
    y = _LMApply.apply(x.reshape(O, shape[d], I), plan, 'bwd' if adjoint else 'fwd', bool(out_real), K_in)
    return y.reshape(shape[:d] + (y.shape[1],) + shape[d + 1:])


# ---------------------------------------------------------------------------------------
# redundant / per-baseline visibility model term: out = vis +- model[red[b], tmap[t]] (csrc/redvis.hip)
# ---------------------------------------------------------------------------------------
def _csr(index, N):
    """(offsets [N + 1], members) of a map index [n] -> [0, N): the members of every target in ascending position"""
    off = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(index, minlength=N), out=off[1:])
    return off.astype(np.int32), np.argsort(index, kind='stable').astype(np.int32)


class RedVisPlan(_IndexPlan):
    """
    Index tables of one (baseline set, time set) of rime_redvis_fwd / rime_redvis_bwd, built with numpy on the host (no GPU
    needed) and cached per device as int32 tensors: `red` [Nbl], the group (model row) of every baseline; `tmap` [Nt], the
    model time of every time (None with Ntm: the identity over Ntm times); and the two CSR tables of the backward reduction,
    goff [Nred + 1] / gmem [Nbl] (baselines of every group, ascending) and toff [Ntm + 1] / tmem [Nt] (times of every model
    time, ascending).  A `red` entry outside [0, Nred) or a `tmap` entry outside [0, Ntm) is a ValueError.
    """
    _TABLES = ('red', 'tmap', 'goff', 'gmem', 'toff', 'tmem')

    def __init__(self, red, Nred, tmap=None, Ntm=None):
        red = _host_array(red, flat=True)
        if tmap is None:
            if Ntm is None:
                raise ValueError('RedVisPlan needs tmap or, for the identity, Ntm')
            tmap, self.identity_t = np.arange(int(Ntm)), True
        else:
            tmap, self.identity_t = _host_array(tmap, flat=True), False
            if Ntm is None:
                raise ValueError('RedVisPlan needs Ntm with tmap')
        for name, a in (('red', red), ('tmap', tmap)):
            if a.size == 0 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError('%s must be a non-empty integer array' % name)
        self.Nred, self.Ntm, self.Nbl, self.Nt = int(Nred), int(Ntm), int(red.size), int(tmap.size)
        if self.Nred <= 0 or red.min() < 0 or red.max() >= self.Nred:
            raise ValueError('red entry outside [0, %d)' % self.Nred)
        if self.Ntm <= 0 or tmap.min() < 0 or tmap.max() >= self.Ntm:
            raise ValueError('tmap entry outside [0, %d)' % self.Ntm)
        self.red, self.tmap = red.astype(np.int32), tmap.astype(np.int32)
        self.goff, self.gmem = _csr(red, self.Nred)
        self.toff, self.tmem = _csr(tmap, self.Ntm)
        self.max_members = int(np.diff(self.goff).max())


def _redvis_bwd_call(plan, gout, sign):
    """gmodel [NP, NP, Nred, Ntm, Nf] of a contiguous gout [NP, NP, Nbl, Nt, Nf]: every element written by the kernel"""
    NP, _, Nbl, Nt, Nf = gout.shape
    code, _ = _real_dtype(gout)
    T = plan.tables(gout.device)
    gm = torch.empty((NP, NP, plan.Nred, plan.Ntm, Nf), dtype=gout.dtype, device=gout.device)
    rc = lib.rime_redvis_bwd(code, NP, _cptr(gout), _ptr(T['goff']), _ptr(T['gmem']), _ptr(T['toff']),
                             _ptr(T['tmem']), Nbl, Nt, Nf, plan.Nred, plan.Ntm, sign, _cptr(gm), _stream())
    check(rc, 'rime_redvis_bwd')
    return gm


class _RedVis(torch.autograd.Function):
    """out = vis + sign * model[:, :, red][:, :, :, tmap] in one pass; backward: gvis = gout itself, gmodel by the segmented
    fixed-order reduction"""
    @staticmethod
    def forward(ctx, vis, model, plan, sign):
        _require_cuda(vis, model)
        assert model.is_complex() and model.ndim == 5, 'complex model of shape (Npol, Npol, Nred, Ntimes, Nfreqs)'
        NP, Nf = model.shape[0], model.shape[4]
        assert NP in (1, 2) and model.shape[1] == NP, 'Npol must be 1 or 2'
        if tuple(model.shape[2:4]) != (plan.Nred, plan.Ntm):
            raise ValueError('model of %d rows and %d times, the plan has %d and %d' % (tuple(model.shape[2:4]) + (plan.Nred, plan.Ntm)))
        shape = (NP, NP, plan.Nbl, plan.Nt, Nf)
        v = None
        if vis is not None:
            assert vis.is_complex(), 'complex visibilities'
            if tuple(vis.shape) != shape:
                raise ValueError('vis of shape %s, the plan and the model give %s' % (tuple(vis.shape), shape))
            v = vis.detach().contiguous()
        dtype = v.dtype if v is not None else model.dtype
        m = model.detach().resolve_conj()
        if m.dtype != dtype:
            m = m.to(dtype)
        st = m.stride()
        if min(st) < 0 or (NP == 2 and st[0] != 2 * st[1]):
            m = m.contiguous()
            st = m.stride()
        code, _ = _real_dtype(m)
        T = plan.tables(m.device)
        out = torch.empty(shape, dtype=dtype, device=m.device)
        rc = lib.rime_redvis_fwd(code, NP, _cptr(v), _cptr(m), _ptr(T['red']), _ptr(None if plan.identity_t else T['tmap']),
                                 plan.Nbl, plan.Nt, Nf, plan.Nred, plan.Ntm, st[1], st[2], st[3], st[4], sign, _cptr(out), _stream())
        check(rc, 'rime_redvis_fwd')
        ctx.plan, ctx.sign, ctx.mdtype = plan, sign, model.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        gm = None
        if ctx.needs_input_grad[1]:
            gm = _redvis_bwd_call(ctx.plan, _dense(gout), ctx.sign)
            if gm.dtype != ctx.mdtype:
                gm = gm.to(ctx.mdtype)
        return (gout if ctx.needs_input_grad[0] else None), gm, None, None


def redvis(vis, model, plan, undo=False):
    """
    out[p, q, b, t, f] = vis[p, q, b, t, f] +- model[p, q, red[b], tmap[t], f] (minus with undo) in one launch of
    rime_redvis_fwd: vis (Npol, Npol, Nbl, Nt, Nf) complex or None (the inflated model alone), model (Npol, Npol, Nred, Ntm, Nf)
    complex, any view with non-negative strides (an expanded axis is read in place), plan a RedVisPlan.  Differentiable once
    with respect to both: the gradient of vis is the incoming gradient itself, that of the model the segmented reduction of
    rime_redvis_bwd, whose summation order is fixed by the plan (bit-identical from run to run).  No CPU path.
    """
    return _RedVis.apply(vis, model, plan, -1 if undo else 1)


# ---------------------------------------------------------------------------------------
# LST alignment: rephasing, weighting and the average of the integrations of every bin in one pass (csrc/lstbin.hip)
# ---------------------------------------------------------------------------------------
class TimeAvgPlan(_IndexPlan):
    """
    Bin table of rime_vis_timeavg_fwd / rime_vis_timeavg_bwd, built with numpy on the host (no GPU needed), validated here on
    the host copies and cached per device as int32 tensors.  bins: a list with the time indices of every bin (any integer
    sequences; an empty entry is an empty bin); a time in no bin is dropped, a time may be in several bins or several times
    in one.  Forward CSR: bin_ptr [Nbin + 1], members [Nmem]: the members of a bin are summed in the order given.  Transposed
    table of the backward gather: t_ptr [Nt + 1], t_pos [Nmem] (the table positions that hold every time, ascending) and
    pos_bin [Nmem] (the bin of every table position).  A member outside [0, Nt) is a ValueError.
    """
    _TABLES = ('bin_ptr', 'members', 't_ptr', 't_pos', 'pos_bin')

    def __init__(self, bins, Nt):
        self.Nt, self.Nbin = int(Nt), len(bins)
        if self.Nt < 0:
            raise ValueError('Nt must not be negative')
        rows = [_host_array(b, flat=True, integer='time indices must be integers').astype(np.int64) for b in bins]
        self.bin_ptr = np.zeros(self.Nbin + 1, dtype=np.int32)
        if rows:
            np.cumsum([r.size for r in rows], out=self.bin_ptr[1:])
        members = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        if members.size and (members.min() < 0 or members.max() >= self.Nt):
            raise ValueError('time index outside [0, %d)' % self.Nt)
        self.Nmem = int(members.size)
        self.members = members.astype(np.int32)
        self.pos_bin = np.repeat(np.arange(self.Nbin), np.diff(self.bin_ptr)).astype(np.int32)
        self.t_ptr, self.t_pos = _csr(members, self.Nt) if self.Nt else (np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32))


def _host_ip(a):
    return a.ctypes.data_as(_lib._ip)


def _timeavg_tau(tau, freqs, plan, Nbl, Nf, by_member, dev):
    if tau is None:
        return None, None
    if freqs is None:
        raise ValueError('rephasing needs freqs')
    tau = torch.as_tensor(tau, dtype=torch.float64).to(dev).contiguous()
    fr = torch.as_tensor(freqs).detach().to(device=dev, dtype=torch.float64).contiguous()
    if tuple(tau.shape) != (Nbl, plan.Nmem if by_member else plan.Nt):
        raise ValueError('tau of shape %s, expected %s' % (tuple(tau.shape), (Nbl, plan.Nmem if by_member else plan.Nt)))
    if tuple(fr.shape) != (Nf,):
        raise ValueError('freqs of shape %s, expected (%d,)' % (tuple(fr.shape), Nf))
    return tau, fr


class _VisTimeAvg(torch.autograd.Function):
    """(avg, sum_w, avg_cov, avg_flag) of rime_vis_timeavg_fwd; backward: the gradient of the data alone, by
    rime_vis_timeavg_bwd (weights, tau and cov receive no gradient)"""
    @staticmethod
    def forward(ctx, data, plan, wgts, cov, flags, tau, freqs, by_member):
        _require_cuda(data, wgts, cov, flags)
        assert data.is_complex() and data.ndim >= 3, 'complex data of shape (..., Nbl, Ntimes, Nfreqs)'
        lead, (Nbl, Nt, Nf) = tuple(data.shape[:-3]), data.shape[-3:]
        if Nt != plan.Nt:
            raise ValueError('data of %d times, the plan has %d' % (Nt, plan.Nt))
        Npp = int(np.prod(lead)) if lead else 1
        d = _dense(data)
        code, rdt = _real_dtype(d)
        dev = d.device

        def full(x, dtype):
            if x is None:
                return None
            x = x.detach()
            if x.dtype != dtype:
                x = x.to(dtype)
            return x.expand(d.shape).contiguous()

        w, c, fl = full(wgts, rdt), full(cov, rdt), full(flags, torch.bool)
        tau, fr = _timeavg_tau(tau, freqs, plan, Nbl, Nf, by_member, dev)
        T = plan.tables(dev)
        oshape = lead + (Nbl, plan.Nbin, Nf)
        avg = torch.empty(oshape, dtype=d.dtype, device=dev)
        sum_w = torch.empty(oshape, dtype=rdt, device=dev)
        avg_cov = torch.empty(oshape, dtype=rdt, device=dev) if c is not None else None
        avg_flag = torch.empty(oshape, dtype=torch.bool, device=dev) if fl is not None else None
        rc = lib.rime_vis_timeavg_fwd(code, _cptr(d), _ptr(w), _ptr(c), _ptr(fl), _ptr(tau), int(bool(by_member)),
                                      _ptr(fr), _ptr(T['bin_ptr']), _ptr(T['members']), _host_ip(plan.bin_ptr),
                                      _host_ip(plan.members), Npp, Nbl, Nt, Nf, plan.Nbin, plan.Nmem,
                                      _cptr(avg), _ptr(sum_w), _ptr(avg_cov), _ptr(avg_flag), _stream())
        check(rc, 'rime_vis_timeavg_fwd')
        ctx.plan, ctx.by_member, ctx.shape, ctx.ddtype = plan, bool(by_member), tuple(d.shape), data.dtype
        ctx.save_for_backward(w, sum_w, tau, fr)
        outs = (avg, sum_w, avg_cov, avg_flag)
        ctx.mark_non_differentiable(*[o for o in outs[1:] if o is not None])
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gavg, *unused):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        plan = ctx.plan
        w, sum_w, tau, fr = ctx.saved_tensors
        code, rdt = _real_dtype(sum_w)
        g = _dense(gavg, _lib_cdtype(rdt))
        Nbl, Nt, Nf = ctx.shape[-3:]
        Npp = int(np.prod(ctx.shape[:-3])) if len(ctx.shape) > 3 else 1
        T = plan.tables(g.device)
        gd = torch.empty(ctx.shape, dtype=g.dtype, device=g.device)
        rc = lib.rime_vis_timeavg_bwd(code, _cptr(g), _ptr(w), _ptr(sum_w), _ptr(tau), int(ctx.by_member),
                                      _ptr(fr), _ptr(T['t_ptr']), _ptr(T['t_pos']), _ptr(T['pos_bin']), _host_ip(plan.t_ptr),
                                      _host_ip(plan.t_pos), _host_ip(plan.pos_bin), Npp, Nbl, Nt, Nf, plan.Nbin, plan.Nmem,
                                      _cptr(gd), _stream())
        check(rc, 'rime_vis_timeavg_bwd')
        if gd.dtype != ctx.ddtype:
            gd = gd.to(ctx.ddtype)
        return (gd,) + (None,) * 7


def vis_timeavg(data, plan, wgts=None, cov=None, flags=None, tau=None, freqs=None, tau_by_member=False):
    """
    (avg, sum_w, avg_cov, avg_flag) of the bins of `plan` (a TimeAvgPlan) in one launch of rime_vis_timeavg_fwd:
        sum_w = sum w,  avg = sum w V exp(2 pi i freqs tau) / max(sum_w, 1e-40),  avg_cov = sum w^2 cov / max(sum_w, 1e-40)^2,
        avg_flag = every member flagged
    over the members of every bin in table order.  data (..., Nbl, Ntimes, Nfreqs) complex64 / complex128; wgts, cov (real)
    and flags (bool) broadcast against it (None: uniform weights, no avg_cov, no avg_flag); tau float64 (Nbl, Ntimes), or
    (Nbl, Nmem) -- one delay [s] per table position -- with tau_by_member (None: no rephasing), freqs (Nfreqs,) [Hz].
    Differentiable once with respect to the DATA only: weights, tau and cov receive no gradient.  The summation order is
    fixed by the plan (bit-identical from run to run).  No CPU path.
    """
    return _VisTimeAvg.apply(data, plan, wgts, cov, flags, tau, freqs, tau_by_member)


def rephase_phasor(tau, freqs, dtype=torch.complex64):
    """exp(2 pi i freqs tau) of shape tau.shape + (Nfreqs,) from the data-less mode of rime_vis_timeavg_fwd: tau float64
    (Nbl, Ntimes) [s] on the GPU, the phase reduced in float64 before sine and cosine are taken in the precision of `dtype`"""
    tau = torch.as_tensor(tau, dtype=torch.float64)
    freqs = torch.as_tensor(freqs)
    _require_cuda(tau, freqs)
    assert tau.ndim == 2 and dtype in (torch.complex64, torch.complex128)
    Nbl, Nt = tau.shape
    Nf = freqs.numel()
    plan = TimeAvgPlan(np.arange(Nt)[:, None], Nt)
    tau, fr = _timeavg_tau(tau, freqs.reshape(-1), plan, Nbl, Nf, False, tau.device)
    T = plan.tables(tau.device)
    out = torch.empty((Nbl, Nt, Nf), dtype=dtype, device=tau.device)
    code, _ = _real_dtype(out)
    rc = lib.rime_vis_timeavg_fwd(code, _ptr(None), _ptr(None), _ptr(None), _ptr(None), _ptr(tau), 0, _ptr(fr), _ptr(T['bin_ptr']),
                                  _ptr(T['members']), _host_ip(plan.bin_ptr), _host_ip(plan.members), 1, Nbl, Nt, Nf, Nt, Nt,
                                  _cptr(out), _ptr(None), _ptr(None), _ptr(None), _stream())
    check(rc, 'rime_vis_timeavg_fwd')
    return out


# ---------------------------------------------------------------------------------------
# lightcone sampling of periodic simulation boxes in one launch (csrc/lcone.hip)
# ---------------------------------------------------------------------------------------
LCONE_INTERP = {'nearest': 0, 'linear': 1}
_LCONE_SPHERE, _LCONE_PLANE = 0, 1


def lcone_sample(sims, dc, cube_idx, weight, S, sim_res, vec=None, roll=(0, 0, 0), interp='nearest'):
    """
    out[i, p] = sum_{s < S} weight[i, s] sample(sims[cube_idx[i, s]], vec[:, p] * dc[i] / sim_res) in one launch of
    rime_lcone_fwd: sims (Nsim, Nx, Ny, Nz) float32 / float64 on the GPU; dc (Nr,) float64, cube_idx (Nr, 3) int32 and weight
    (Nr, 3) float64 host arrays (the radial stencil table, S = 1 ... 3 columns used); vec (3, Npix) float64 host array or GPU
    tensor, or None for the plane mode (out (Nr, Nx, Ny), only z = dc / sim_res sampled); roll: three ints, any sign; interp
    'nearest' or 'linear'.  Returns (Nr, Npix) in the dtype of sims.  Not differentiable (the reference function is not
    either).  No CPU path.
    """
    _require_cuda(sims)
    assert sims.ndim == 4 and sims.dtype in (torch.float32, torch.float64)
    dev = sims.device
    sims = _dense(sims)
    code, _ = _real_dtype(sims)
    Nsim, Nx, Ny, Nz = sims.shape
    dc = np.ascontiguousarray(dc, dtype=np.float64).reshape(-1)
    Nr = dc.size
    cube_idx = np.ascontiguousarray(cube_idx, dtype=np.int32).reshape(Nr, 3)
    weight = np.ascontiguousarray(weight, dtype=np.float64).reshape(Nr, 3)
    if vec is None:
        mode, Npix, vdev, shape = _LCONE_PLANE, Nx * Ny, None, (Nr, Nx, Ny)
    else:
        vdev = torch.as_tensor(vec, dtype=torch.float64).to(dev).contiguous()
        assert vdev.ndim == 2 and vdev.shape[0] == 3
        mode, Npix, shape = _LCONE_SPHERE, vdev.shape[1], (Nr, vdev.shape[1])
    rx, ry, rz = (int(r) % n for r, n in zip(roll, (Nx, Ny, Nz)))
    out = torch.empty(shape, dtype=sims.dtype, device=dev)
    if out.numel() == 0:
        return out
    d_dc, d_idx, d_w = torch.as_tensor(dc).to(dev), torch.as_tensor(cube_idx).to(dev), torch.as_tensor(weight).to(dev)
    rc = lib.rime_lcone_fwd(code, mode, LCONE_INTERP[interp], int(S), _ptr(sims), _ptr(vdev), _ptr(d_dc), _ptr(d_idx),
                            _ptr(d_w), _host_ip(cube_idx), float(sim_res), rx, ry, rz, Nsim, Nx, Ny, Nz, Nr, Npix,
                            _ptr(out), _stream())
    check(rc, 'rime_lcone_fwd')
    return out


# ---------------------------------------------------------------------------------------
# antenna mutual coupling: W = E V E^H on one batched complex product kernel (csrc/coupling.hip)
# ---------------------------------------------------------------------------------------
COUPLING_CONJ = 1 << 30                          # table word: the row is read conjugated (ftab: no conjugated reader)
COUPLING_PROD = {'both': 0, 'left': 1, 'right': 2}
_COUPLING_FWD, _COUPLING_BWD, _COUPLING_EXPAND_BWD = 0, 1, 2


class CouplingPlan(_IndexPlan):
    """
    Tables of rime_coupling_fwd / rime_coupling_bwd for one (antenna order, baseline list), built and range-checked with numpy
    on the host (no GPU needed) and cached per device as int32 tensors.
      table     (N, N) integers: entry (a, b) of the visibility matrix is data[row] for the word `row`, conj(data[row]) for
                `row | COUPLING_CONJ`, zero for -1
      out_rows  (Nout,) flat matrix positions a * N + b of the output rows, in output order
      Nbl       rows of the data
    Derived: `otab` (N, N), the output row of every matrix entry or -1, and `ftab` (N, N), at the entry that reads a data row
    unconjugated the row itself, with COUPLING_CONJ set when no entry reads it conjugated (its gradient is then the single
    term), -1 elsewhere.  ValueError for a table that is not square, a word outside {-1} U [0, Nbl) (| COUPLING_CONJ), a row
    read twice in the same sense or only conjugated, a row read conjugated anywhere but at the transpose of the entry that
    reads it plain (the folded gradient pairs (a, b) with (b, a)), an output position outside the matrix or named twice.
    """
    _TABLES = ('table', 'otab', 'ftab')

    def __init__(self, table, out_rows, Nbl):
        table, out_rows = _host_array(table), _host_array(out_rows, flat=True)
        if table.ndim != 2 or table.shape[0] != table.shape[1] or table.shape[0] < 1 or not np.issubdtype(table.dtype, np.integer):
            raise ValueError('table must be a square integer matrix')
        if out_rows.size < 1 or not np.issubdtype(out_rows.dtype, np.integer):
            raise ValueError('out_rows must be a non-empty integer array')
        table = table.astype(np.int64)
        self.N, self.Nbl, self.Nout = int(table.shape[0]), int(Nbl), int(out_rows.size)
        if not 1 <= self.Nbl < COUPLING_CONJ:
            raise ValueError('Nbl must be in [1, 2^30)')
        null = table == -1
        if (table[~null] < 0).any():
            raise ValueError('a table word is -1 (null) or a row with an optional conjugate bit')
        row = np.where(null, -1, table & (COUPLING_CONJ - 1))
        conj = ~null & ((table & COUPLING_CONJ) != 0)
        if ((table & ~np.int64(2 * COUPLING_CONJ - 1)) != 0)[~null].any() or (row[~null] >= self.Nbl).any():
            raise ValueError('table row outside [0, %d)' % self.Nbl)
        plain = ~null & ~conj
        nplain, nconj = np.bincount(row[plain], minlength=self.Nbl), np.bincount(row[conj], minlength=self.Nbl)
        if nplain.max(initial=0) > 1 or nconj.max(initial=0) > 1:
            raise ValueError('a data row is read twice in the same sense')
        if ((nconj > 0) & (nplain == 0)).any():
            raise ValueError('a data row is read only conjugated')
        if (conj & ~((row.T == row) & plain.T)).any():
            raise ValueError('the conjugated reader of a data row must be the transpose of its plain reader')
        if out_rows.min() < 0 or out_rows.max() >= self.N * self.N or np.unique(out_rows).size != out_rows.size:
            raise ValueError('out_rows must be distinct positions in [0, %d)' % (self.N * self.N))
        self.table = table.astype(np.int32)
        otab = np.full(self.N * self.N, -1, dtype=np.int32)
        otab[out_rows] = np.arange(self.Nout, dtype=np.int32)
        self.otab = otab.reshape(self.N, self.N)
        self.ftab = np.where(plain, row | np.where(nconj[np.maximum(row, 0)] == 0, COUPLING_CONJ, 0), -1).astype(np.int32)
        self.out_rows = out_rows.astype(np.int64)
        self.unread = bool((nplain == 0).any())           # rows of the data outside the matrix: their gradient is zero


def _coupling_operands(coupling, dly, dtype, Nf=None):
    """(x, dly, N, Tm, Fm, Nf) contiguous in `dtype`: coupling (N, N, Tm, Fm), dly (N, N, 1, Nf) or None"""
    assert coupling.is_complex() and coupling.ndim == 4 and coupling.shape[0] == coupling.shape[1], \
        'complex coupling of shape (Nant, Nant, Ntimes | 1, Nfreqs | 1)'
    x = _dense(coupling, dtype)
    N, _, Tm, Fm = x.shape
    d = None
    if dly is not None:
        assert dly.is_complex() and dly.ndim == 4 and tuple(dly.shape[:3]) == (N, N, 1), 'complex dly of shape (Nant, Nant, 1, Nfreqs)'
        d = _dense(dly, dtype)
        if Nf is not None and d.shape[3] != Nf:
            raise ValueError('dly of %d channels, data of %d' % (d.shape[3], Nf))
        Nf = d.shape[3]
    elif Nf is None:
        Nf = Fm
    return x, d, N, Tm, Fm, Nf


def _coupling_fwd_call(coupling, dly, data, plan, add_I, prod, out=None):
    """W rows (Nout, Nt, Nf) of a contiguous complex data (Nbl, Nt, Nf); `out`: a contiguous tensor to write into"""
    Nbl, Nt, Nf = data.shape
    x, d, N, Tm, Fm, _ = _coupling_operands(coupling, dly, data.dtype, Nf)
    if N != plan.N or Nbl != plan.Nbl:
        raise ValueError('coupling of %d antennas and data of %d rows, the plan has %d and %d' % (N, Nbl, plan.N, plan.Nbl))
    if Tm not in (1, Nt) or Fm not in (1, Nf):
        raise ValueError('coupling of (%d, %d) times and channels against data of (%d, %d)' % (Tm, Fm, Nt, Nf))
    code, _ = _real_dtype(data)
    T = plan.tables(data.device)
    if out is None:
        out = torch.empty((plan.Nout, Nt, Nf), dtype=data.dtype, device=data.device)
    assert out.is_contiguous() and tuple(out.shape) == (plan.Nout, Nt, Nf) and out.dtype == data.dtype
    ws, nbytes = _workspace(lib.rime_coupling_workspace(code, N, Nt, Nf, Tm, Fm, COUPLING_PROD[prod], _COUPLING_FWD), data.device)
    rc = lib.rime_coupling_fwd(code, _cptr(x), _cptr(d), _cptr(data), _ptr(T['table']), _ptr(T['otab']), N, Nbl, plan.Nout, Nt, Nf,
                               Tm, Fm, int(bool(add_I)), COUPLING_PROD[prod], _cptr(out), _ptr(ws), nbytes, _stream())
    check(rc, 'rime_coupling_fwd')
    return out


class _CouplingApply(torch.autograd.Function):
    """W = E V E^H (or E V, V E^H) with E = [I] + coupling o dly; saves coupling and data only, T = E V is recomputed"""
    @staticmethod
    def forward(ctx, coupling, dly, data, plan, add_I, prod):
        _require_cuda(coupling, dly, data)
        assert data.is_complex() and data.ndim == 3, 'complex data of shape (Nbls, Ntimes, Nfreqs)'
        if prod not in COUPLING_PROD:
            raise ValueError("prod must be 'both', 'left' or 'right'")
        v = _dense(data)
        out = _coupling_fwd_call(coupling, dly, v, plan, add_I, prod)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(coupling.detach(), dly.detach() if dly is not None else None, v)
            ctx.plan, ctx.add_I, ctx.prod, ctx.xdtype, ctx.ddtype = plan, bool(add_I), prod, coupling.dtype, data.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        coupling, dly, v = ctx.saved_tensors
        plan = ctx.plan
        Nbl, Nt, Nf = v.shape
        x, d, N, Tm, Fm, _ = _coupling_operands(coupling, dly, v.dtype, Nf)
        g = _dense(gout, v.dtype)
        code, _ = _real_dtype(v)
        T = plan.tables(v.device)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gd = None
        if ctx.needs_input_grad[2]:
            gd = torch.zeros_like(v) if plan.unread else torch.empty_like(v)
        prod = COUPLING_PROD[ctx.prod]
        ws, nbytes = _workspace(lib.rime_coupling_workspace(code, N, Nt, Nf, Tm, Fm, prod, _COUPLING_BWD), v.device)
        rc = lib.rime_coupling_bwd(code, _cptr(x), _cptr(d), _cptr(v), _cptr(g), _ptr(T['table']), _ptr(T['otab']),
                                   _ptr(T['ftab']), N, Nbl, plan.Nout, Nt, Nf, Tm, Fm, int(ctx.add_I), prod,
                                   _cptr(gd), _cptr(gx), _ptr(ws), nbytes, _stream())
        check(rc, 'rime_coupling_bwd')
        if gx is not None and gx.dtype != ctx.xdtype:
            gx = gx.to(ctx.xdtype)
        if gd is not None and gd.dtype != ctx.ddtype:
            gd = gd.to(ctx.ddtype)
        return gx, None, gd, None, None, None


class _CouplingExpand(torch.autograd.Function):
    """the double-path matrix E = [I] + Xd + Xd Xd, Xd = coupling o dly, as a dense (N, N, Tm, Nf) tensor"""
    @staticmethod
    def forward(ctx, coupling, dly, add_I):
        _require_cuda(coupling, dly)
        x, d, N, Tm, Fm, Nf = _coupling_operands(coupling, dly, coupling.dtype)
        code, _ = _real_dtype(x)
        E = torch.empty((N, N, Tm, Nf), dtype=x.dtype, device=x.device)
        rc = lib.rime_coupling_expand(code, _cptr(x), _cptr(d), N, Tm, Nf, Tm, Fm, int(bool(add_I)), _cptr(E), _stream())
        check(rc, 'rime_coupling_expand')
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x, d)
        return E

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gE):
        x, d = ctx.saved_tensors
        N, _, Tm, Fm = x.shape
        Nf = gE.shape[3]
        g = _dense(gE, x.dtype)
        code, _ = _real_dtype(x)
        gx = torch.empty_like(x)
        ws, nbytes = _workspace(lib.rime_coupling_workspace(code, N, Tm, Nf, Tm, Fm, 0, _COUPLING_EXPAND_BWD), x.device)
        rc = lib.rime_coupling_expand_bwd(code, _cptr(x), _cptr(d), _cptr(g), N, Tm, Nf, Tm, Fm, _cptr(gx), _ptr(ws), nbytes,
                                          _stream())
        check(rc, 'rime_coupling_expand_bwd')
        return gx, None, None


def coupling_expand(coupling, dly=None, add_I=True):
    """E = [I] + Xd + Xd Xd with Xd = coupling o dly (double-path coupling) on the product kernel of coupling_apply: coupling
    (N, N, Tm, Fm) complex, dly (N, N, 1, Nf) or None -> (N, N, Tm, Nf | Fm).  Differentiable once in coupling.  No CPU path."""
    return _CouplingExpand.apply(coupling, dly, add_I)


def coupling_apply(coupling, dly, data, table, out_rows=None, add_I=True, prod='both', double=False):
    """
    Mutual coupling of visibilities, W = E V E^H (prod 'both'), E V ('left') or V E^H ('right') per time and channel, with
    E = [I] + coupling o dly built on the fly, V read from `data` through the matrix table and only the output rows written
    (rime_coupling_fwd; nothing of size (N^2, Nt, Nf) is gathered or saved).
      coupling (N, N, Tm, Fm) complex, Tm in {1, Nt}, Fm in {1, Nf};  dly (N, N, 1, Nf) complex or None
      data     (Nbl, Nt, Nf) complex64 / complex128
      table    a CouplingPlan, or the (N, N) integer table with `out_rows`, the flat matrix positions of the output rows
      double   E = [I] + Xd + Xd Xd, Xd = coupling o dly, formed first as a dense tensor (coupling_expand)
    Differentiable once in coupling and data: gdata = fold(E^H G E), gcoupling = (G E V^H + G^H E V) o conj(dly) summed over
    the broadcast axes, every sum by one thread in a fixed order (bit-identical from run to run).  No CPU path.
    """
    plan = table if isinstance(table, CouplingPlan) else CouplingPlan(table, out_rows, data.shape[0])
    if double:
        E = _CouplingExpand.apply(coupling.to(data.dtype), dly, add_I)
        return _CouplingApply.apply(E, None, data, plan, False, prod)
    return _CouplingApply.apply(coupling, dly, data, plan, add_I, prod)


# ---------------------------------------------------------------------------------------
# mutual coupling of redundant visibilities: Vc = A(eps) Vr + B(eps) conj(Vr) on a sparse entry list (csrc/redcoupling.hip)
# ---------------------------------------------------------------------------------------
REDCOUPLING_SEG = 64                             # words of a segment of a term's list in the gradient of the coefficients
REDCOUPLING_FLAG = 1 << 30                       # column word: the visibility is read conjugated; term word: role b


class RedCouplingPlan(_IndexPlan):
    """
    Tables of rime_redcoupling_fwd / _bwd_data / _bwd_coupling, built and range-checked with numpy on the host (no GPU
    needed) and cached per device as int32 tensors.  Entry e = (row[e], col[e], conj[e], a[e], b[e]) adds
        (a >= 0 ? C[a] : 1) (b >= 0 ? conj(C[b]) : 1) (conj ? conj(data[col]) : data[col])        C = coupling o dly
    to output row[e]; -1 for a or b means no factor.  The entries are kept sorted by row (stable), and three CSR orderings of
    them, each ascending: `roff` [Nout + 1] by output row; `coff` [Nin + 1] / `cmem` [Nent] by input column; `toff`
    [Nterms + 1] / `tmem` by coupling term, the words `e` (the term is a[e]) and `e | REDCOUPLING_FLAG` (it is b[e]), an entry
    with a == b under both.  Every term's list is cut into segments of `seg` words: `segterm`, `segstart` [Nseg] and `tsoff`
    [Nterms + 1], the segments of every term.  ValueError for arrays of different lengths, no entry, a row outside [0, Nout),
    a column outside [0, Nin), a or b outside [-1, Nterms), a conj outside {0, 1}, 2^30 entries or more.
    """
    def __init__(self, row, col, conj, a, b, Nout, Nin, Nterms, seg=REDCOUPLING_SEG):
        arrs = []
        for name, x in (('row', row), ('col', col), ('conj', conj), ('a', a), ('b', b)):
            x = _host_array(x, flat=True)
            if x.dtype == bool:
                x = x.astype(np.int64)
            if x.size and not np.issubdtype(x.dtype, np.integer):
                raise ValueError('%s must be an integer array' % name)
            arrs.append(x.astype(np.int64))
        row, col, conj, a, b = arrs
        self.Nout, self.Nin, self.Nterms, self.seg = int(Nout), int(Nin), int(Nterms), int(seg)
        self.Nent = int(row.size)
        if any(x.size != self.Nent for x in arrs):
            raise ValueError('row, col, conj, a and b must have one length')
        if not 1 <= self.Nent < REDCOUPLING_FLAG:
            raise ValueError('the plan needs between 1 and 2^30 - 1 entries')
        if min(self.Nout, self.Nin, self.Nterms) < 1 or max(self.Nout, self.Nin) >= REDCOUPLING_FLAG or not 1 <= self.seg <= 1 << 20:
            raise ValueError('Nout, Nin, Nterms must be positive and seg in [1, 2^20]')
        if row.min() < 0 or row.max() >= self.Nout:
            raise ValueError('entry row outside [0, %d)' % self.Nout)
        if col.min() < 0 or col.max() >= self.Nin:
            raise ValueError('entry column outside [0, %d)' % self.Nin)
        if min(a.min(), b.min()) < -1 or max(a.max(), b.max()) >= self.Nterms:
            raise ValueError('coupling term outside [-1, %d)' % self.Nterms)
        if conj.min() < 0 or conj.max() > 1:
            raise ValueError('conj must be 0 or 1')
        order = np.argsort(row, kind='stable')
        row, col, conj, a, b = (x[order] for x in (row, col, conj, a, b))
        self.row, self.col, self.conj, self.a, self.b = row, col, conj, a, b
        self.ent = np.stack([row, col | (conj * REDCOUPLING_FLAG), a, b], axis=1).astype(np.int32)
        self.roff = _csr(row, self.Nout)[0]
        self.coff, self.cmem = _csr(col, self.Nin)
        term = np.stack([a, b], axis=1).reshape(-1)                         # (entry, role) in ascending order
        word = np.stack([np.arange(self.Nent), np.arange(self.Nent) | REDCOUPLING_FLAG], axis=1).reshape(-1)
        used = term >= 0
        term, word = term[used], word[used]
        self.toff, pos = _csr(term, self.Nterms)
        self.tmem = word[pos].astype(np.int32)
        self.Nmem = int(self.tmem.size)
        count = np.diff(self.toff.astype(np.int64))
        nseg = (count + self.seg - 1) // self.seg
        tsoff = np.zeros(self.Nterms + 1, dtype=np.int64)
        np.cumsum(nseg, out=tsoff[1:])
        self.tsoff, self.Nseg = tsoff.astype(np.int32), int(tsoff[-1])
        self.segterm = np.repeat(np.arange(self.Nterms), nseg).astype(np.int32)
        self.segstart = (self.toff[self.segterm] + (np.arange(self.Nseg) - tsoff[self.segterm]) * self.seg).astype(np.int32)
        self.term_counts = count

    _TABLES = ('ent', 'roff', 'coff', 'cmem', 'toff', 'tmem', 'segterm', 'segstart', 'tsoff')


def _redcoupling_operands(coupling, dly, data, plan):
    """(x, d, v, Tm, Fm) contiguous in the dtype of the data"""
    assert data.is_complex() and data.ndim == 3, 'complex data of shape (Nin, Ntimes, Nfreqs)'
    assert coupling.is_complex() and coupling.ndim == 3, 'complex coupling of shape (Nterms, Ntimes | 1, Nfreqs | 1)'
    v = _dense(data)
    Nin, Nt, Nf = v.shape
    x = _dense(coupling, v.dtype)
    Nterms, Tm, Fm = x.shape
    if Nin != plan.Nin or Nterms != plan.Nterms:
        raise ValueError('data of %d rows and coupling of %d terms, the plan has %d and %d' % (Nin, Nterms, plan.Nin, plan.Nterms))
    if Tm not in (1, Nt) or Fm not in (1, Nf):
        raise ValueError('coupling of (%d, %d) times and channels against data of (%d, %d)' % (Tm, Fm, Nt, Nf))
    d = None
    if dly is not None:
        assert dly.is_complex() and tuple(dly.shape) == (Nterms, Nf), 'complex dly of shape (Nterms, Nfreqs)'
        d = _dense(dly, v.dtype)
    return x, d, v, Tm, Fm


class _RedCouplingApply(torch.autograd.Function):
    """out = sum of the plan's entries; saves coupling, dly and data, the coefficients are rebuilt in the backward kernels"""
    @staticmethod
    def forward(ctx, coupling, dly, data, plan):
        _require_cuda(coupling, dly, data)
        x, d, v, Tm, Fm = _redcoupling_operands(coupling, dly, data, plan)
        _, Nt, Nf = v.shape
        code, _ = _real_dtype(v)
        T = plan.tables(v.device)
        out = torch.empty((plan.Nout, Nt, Nf), dtype=v.dtype, device=v.device)
        rc = lib.rime_redcoupling_fwd(code, _cptr(x), _cptr(d), _cptr(v), _ptr(T['ent']), _ptr(T['roff']), plan.Nout, plan.Nin,
                                      plan.Nterms, plan.Nent, Nt, Nf, Tm, Fm, _cptr(out), _stream())
        check(rc, 'rime_redcoupling_fwd')
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, d, v)
            ctx.plan, ctx.xdtype, ctx.ddtype = plan, coupling.dtype, data.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, d, v = ctx.saved_tensors
        plan = ctx.plan
        _, Nt, Nf = v.shape
        _, Tm, Fm = x.shape
        g = _dense(gout, v.dtype)
        code, _ = _real_dtype(v)
        T = plan.tables(v.device)
        dims = (plan.Nout, plan.Nin, plan.Nterms, plan.Nent)
        gx = gd = None
        if ctx.needs_input_grad[2]:
            gd = torch.empty_like(v)
            rc = lib.rime_redcoupling_bwd_data(code, _cptr(x), _cptr(d), _cptr(g), _ptr(T['ent']), _ptr(T['coff']), _ptr(T['cmem']),
                                               *dims, Nt, Nf, Tm, Fm, _cptr(gd), _stream())
            check(rc, 'rime_redcoupling_bwd_data')
            if gd.dtype != ctx.ddtype:
                gd = gd.to(ctx.ddtype)
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            ws, nbytes = _workspace(lib.rime_redcoupling_workspace(code, plan.Nseg, Nt, Nf), v.device)
            seg = [_ptr(T[k]) if plan.Nseg else _ptr(None) for k in ('tmem', 'segterm', 'segstart')]
            rc = lib.rime_redcoupling_bwd_coupling(code, _cptr(x), _cptr(d), _cptr(v), _cptr(g), _ptr(T['ent']), _ptr(T['toff']),
                                                   seg[0], seg[1], seg[2], _ptr(T['tsoff']), *dims, plan.Nmem, plan.Nseg,
                                                   plan.seg, Nt, Nf, Tm, Fm, _cptr(gx), _ptr(ws), nbytes, _stream())
            check(rc, 'rime_redcoupling_bwd_coupling')
            if gx.dtype != ctx.xdtype:
                gx = gx.to(ctx.xdtype)
        return gx, None, gd, None


def redcoupling_apply(coupling, dly, data, plan):
    """
    Coupled visibilities of a redundant model, out[i] = sum over the entries (i, j, conj, a, b) of the RedCouplingPlan of
    (a >= 0 ? C[a] : 1) (b >= 0 ? conj(C[b]) : 1) (conj ? conj(data[j]) : data[j]) with C = coupling o dly built on the fly
    (rime_redcoupling_fwd): no (Nout, Nin, Nt, Nf) matrix is formed.
      coupling (Nterms, Tm, Fm) complex, Tm in {1, Nt}, Fm in {1, Nf};  dly (Nterms, Nf) complex or None
      data     (Nin, Nt, Nf) complex64 / complex128  ->  (Nout, Nt, Nf)
    Differentiable once in coupling and data; every gradient sum runs in an order fixed by the plan, without atomics
    (bit-identical from run to run); columns that nothing reads and terms without an entry get zeros.  No CPU path.
    """
    return _RedCouplingApply.apply(coupling, dly, data, plan)


# ---------------------------------------------------------------------------------------
# sparse learnable mixing of a partly redundant array: out[i] = sum_e c[e] data[col[e]] (csrc/partred.hip)
# ---------------------------------------------------------------------------------------
class PartRedPlan(_IndexPlan):
    """
    Tables of rime_partred_fwd / _bwd_data / _bwd_coeff, built and checked with numpy on the host (no GPU needed) and cached
    per device as int32 tensors.  Entry e adds c[e] * data[cols[e]] to output row rows[e]; the entries of a row are consecutive
    (rows is non-decreasing) and are added in the order given.  `roff` [Nout + 1]: the entries of every row; `col`, `row`
    [Nnz]; `coff` [Nin + 1] / `cmem` [Nnz]: the entries of every column, ascending entry number (the order of the gradient of
    the data).  A row or a column may have no entry.  ValueError for arrays of different lengths or of another kind than
    integer, no entry, a decreasing row, a row outside [0, Nout), a column outside [0, Nin) (a negative one included), the
    same column twice in one row.
    """
    _TABLES = ('roff', 'col', 'row', 'coff', 'cmem')

    def __init__(self, rows, cols, Nout, Nin):
        rows = _host_array(rows, flat=True, integer='rows must be integers').astype(np.int64)
        cols = _host_array(cols, flat=True, integer='cols must be integers').astype(np.int64)
        self.Nout, self.Nin, self.Nnz = int(Nout), int(Nin), int(rows.size)
        if cols.size != self.Nnz:
            raise ValueError('rows and cols must have one length')
        if self.Nnz < 1 or self.Nnz >= 2 ** 31 or min(self.Nout, self.Nin) < 1:
            raise ValueError('the plan needs at least one entry (and fewer than 2^31), one row and one column')
        if rows.min() < 0 or rows.max() >= self.Nout:
            raise ValueError('entry row outside [0, %d)' % self.Nout)
        if cols.min() < 0 or cols.max() >= self.Nin:
            raise ValueError('entry column outside [0, %d)' % self.Nin)
        if (np.diff(rows) < 0).any():
            raise ValueError('the entries of a row must be consecutive: rows must not decrease')
        if np.unique(rows * self.Nin + cols).size != self.Nnz:
            raise ValueError('the same column twice in one row')
        self.row, self.col = rows.astype(np.int32), cols.astype(np.int32)
        self.roff = _csr(rows, self.Nout)[0]
        self.coff, self.cmem = _csr(cols, self.Nin)
        self.max_row, self.max_col = int(np.diff(self.roff).max()), int(np.diff(self.coff).max())


def _partred_view(data, NP):
    """data detached as the kernels read it: any view with non-negative strides whose two pol axes fold into one"""
    v = data.detach().resolve_conj()
    st = v.stride()
    if min(st) < 0 or (NP == 2 and st[0] != 2 * st[1]):
        v = v.contiguous()
    return v


class _PartRed(torch.autograd.Function):
    """out = sum of the plan's entries; saves the data (as the view it came in) and the coefficients"""
    @staticmethod
    def forward(ctx, data, coeff, plan):
        _require_cuda(data, coeff)
        assert data.is_complex() and data.ndim == 5, 'complex data of shape (Npol, Npol, Nin, Ntimes, Nfreqs)'
        NP, _, Nin, Nt, Nf = data.shape
        assert NP in (1, 2) and data.shape[1] == NP, 'Npol must be 1 or 2'
        if Nin != plan.Nin:
            raise ValueError('data of %d baselines, the plan has %d columns' % (Nin, plan.Nin))
        if coeff.is_complex() or tuple(coeff.shape) != (plan.Nnz,):
            raise ValueError('coeff must be real of shape (%d,), one number per entry' % plan.Nnz)
        code, real = _real_dtype(data)
        v, c = _partred_view(data, NP), _dense(coeff, real)
        st = v.stride()
        T = plan.tables(v.device)
        out = torch.empty((NP, NP, plan.Nout, Nt, Nf), dtype=v.dtype, device=v.device)
        rc = lib.rime_partred_fwd(code, NP, _cptr(v), _ptr(c), _ptr(T['roff']), _ptr(T['col']), plan.Nout, Nin, plan.Nnz,
                                  Nt, Nf, st[1], st[2], st[3], st[4], _cptr(out), _stream())
        check(rc, 'rime_partred_fwd')
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(v, c)
            ctx.plan, ctx.cdtype = plan, coeff.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        v, c = ctx.saved_tensors
        plan = ctx.plan
        NP, _, Nin, Nt, Nf = v.shape
        g = _dense(gout, v.dtype)
        code, _ = _real_dtype(v)
        T = plan.tables(v.device)
        dims = (plan.Nout, Nin, plan.Nnz, Nt, Nf)
        gd = gc = None
        if ctx.needs_input_grad[0]:
            gd = torch.empty(tuple(v.shape), dtype=v.dtype, device=v.device)
            rc = lib.rime_partred_bwd_data(code, NP, _cptr(g), _ptr(c), _ptr(T['row']), _ptr(T['coff']), _ptr(T['cmem']), *dims,
                                           _cptr(gd), _stream())
            check(rc, 'rime_partred_bwd_data')
        if ctx.needs_input_grad[1]:
            st = v.stride()
            gc = torch.empty_like(c)
            rc = lib.rime_partred_bwd_coeff(code, NP, _cptr(v), _cptr(g), _ptr(T['roff']), _ptr(T['col']), *dims,
                                            st[1], st[2], st[3], st[4], _ptr(gc), _stream())
            check(rc, 'rime_partred_bwd_coeff')
            if gc.dtype != ctx.cdtype:
                gc = gc.to(ctx.cdtype)
        return gd, gc, None


def partred_inflate(data, coeff, plan):
    """
    out[p, q, i, t, f] = sum over the entries e of row i of the PartRedPlan, in their order, of coeff[e] * data[p, q, col[e], t, f]
    in one launch of rime_partred_fwd: data (Npol, Npol, Nin, Nt, Nf) complex64 / complex128, any view with non-negative
    strides (a sliced, transposed or expanded view is read in place), coeff (Nnz,) real, cast to the real dtype of the data
    -> (Npol, Npol, Nout, Nt, Nf).  A row without entries gives zeros.  Differentiable once in data and coeff, each gradient
    computed only where it is asked for, by a reduction whose order the plan fixes, without atomics (bit-identical from run to
    run); a column that nothing reads gets zeros.  No CPU path.
    """
    return _PartRed.apply(data, coeff, plan)
