"""
Matrix operators for Hessians and inverse Hessians: the counterpart of the reference's hmat.py (BaseMat, DenseMat, DiagMat,
HadamardMat, TriangMat, SparseMat, ZeroMat, OneMat, TransposedMat, PartitionedMat, MatColumn, MatRow, MatSum, MatDict, HierMat,
SolveMat, SolveHierMat) with the products of an operator tree on the grouped mat-vec kernel of csrc/hmat.hip.

An operator tree of DenseMat, DiagMat, SparseMat, ZeroMat, TriangMat leaves, TransposedMat of these and any nesting of
PartitionedMat, HierMat, MatColumn and MatRow is flattened once into a plan: a device table of dense and diagonal tiles at
offsets of the input and output vectors (a low-rank leaf U V is two dense tiles, V from x into a scratch vector in stage 0 and
U from the scratch vector into y in stage 1 -- with an input longer than SPLIT cut into pieces whose partial products are
added by unit diagonal tiles in a stage between; a ZeroMat gives no tile; a HierMat scalar becomes the scale of its tiles), the
row ranges the work-groups own and the tiles of every range in table order.  mat_vec_mul / mat_mat_mul of such a tree are one
rime_hmat_apply call: one launch per stage and four right-hand sides.  A complex vector against the real matrices is its
interleaved real view (two right-hand sides: the matrix is read once).  The plan is cached per (dtype, device, transpose) and
dropped by push, scalar_mul, *=, __setitem__ and pickling.  A plan reads the leaf tensors where they are, so a change made
to a leaf tensor in place is seen -- except where the plan had to make a copy: a leaf of another dtype or device than the
vector, a leaf that is not row-contiguous, the materialised triangle of a TriangMat, and the value of a HierMat scalar.  After
changing such a tensor by hand, call hmat._touch() (or any of the methods above).  OneMat and HadamardMat stay torch expressions; a tree that holds
one (or a SolveMat) is applied leaf by leaf, every flattenable subtree through its own plan.  SolveMat and SolveHierMat solve
with torch.linalg.solve_triangular / solve.  to_dense, diagonal, least_squares and the arithmetic operators are torch
plumbing.  Vectors live on the GPU; there is no CPU path.  Complex-valued matrices are not implemented.

The governing rule: an operator is what its mat_vec_mul does to the identity; to_dense, diagonal, out= (out[:] += result) and
the transposes agree with that.

Deviations from the reference:
  1. SparseMat.to_dense adds Hdiag to the diagonal (the reference adds it to whole columns; PartitionedMat.to_dense over such a
     block follows).
  2. DiagMat.__call__ passes its keywords on (the reference drops them, so HierMat(..., out=) loses the product of a DiagMat leaf).
  3. MatRow.__call__ and MatRow.mat_mat_mul call the method (the reference calls an undefined name).
  4. TriangMat from a 1-D tensor takes its size from the length of that tensor (the reference reads an undefined name).
  5. TriangMat.diagonal reads _diag_idx (the reference reads an undefined attribute).
  6. MatSum adds its products with Python's sum (the reference hands a list to torch.sum); mat_vec_mul is an alias of the
     reference's mat_vec_mult.
  7. out= always means out[:] += result: HierMat and SolveHierMat scale only their own product by `scalar` (the reference
     scales what out held before as well), and MatColumn / MatRow with out= add each product once.
  8. HierMat.mat_vec_mul takes transpose=; HierMat.to_dense(transpose=True) conjugates nothing (real matrices only).
  9. A scalar DiagMat (one value, size > 1) has the dense form value * identity for any size.
 10. scalar_mul and push of a PartitionedMat, MatColumn, MatRow reach a block that is held twice (a symmetric off-diagonal block
     and its transpose) once; the reference scales it twice.  HierMat.scalar_mul replaces `scalar` instead of changing a
     tensor the caller may share.
 11. make_hodlr raises NotImplementedError, as in the reference.

Kept from the reference although they contradict the governing rule (known defects, pinned by no test):
  a. scalar_mul, * and *= of a hermitian SparseMat scale U only: the low-rank part gets scalar^2, Hdiag gets scalar.
  b. A SolveHierMat with both `scalar` and trans_solve applies the scalar in each of its two solves (to_SolveHierMat squares
     the scalar it hands over for that reason).
"""
import ctypes

import numpy as np
import torch

from . import _lib, utils, linalg, paramdict
from .ops import _require_cuda, _stream, _ptr

ROWS = 256            # destination rows of one work-group (csrc/hmat.hip HM_ROWS)
SCRATCH_ROWS = 4      # rows of a plain-form tile into the scratch vector per work-group: one per wave (few, long rows)
SPLIT = 4096          # inputs of the first tile of a low-rank leaf per work-group: a longer input is split into partial sums
MAX_PIECES = 1024
TRANS, DIAG, SRC_SCRATCH = 1, 2, 4
DST_SCRATCH, ACCUMULATE = 1, 2

TILE_DTYPE = np.dtype([('a', '<u8'), ('ld', '<i8'), ('src_off', '<i8'), ('dst_off', '<i8'), ('scale', '<f8'), ('rows', '<i4'),
                       ('cols', '<i4'), ('flags', '<i4'), ('stage', '<i4'), ('reserved', '<i8')])
assert TILE_DTYPE.itemsize == 64

_EPOCH = [0]          # bumped by whatever may change a tree; a plan built in an earlier epoch is rebuilt


def _touch(obj=None):
    _EPOCH[0] += 1
    if obj is not None:
        obj.__dict__.pop('_plans', None)


def _real(dtype):
    return {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(dtype, dtype)


def _code(dtype):
    if dtype == torch.float32:
        return _lib.RIME_F32
    if dtype == torch.float64:
        return _lib.RIME_F64
    raise TypeError('hmat: float32 / float64 (or complex64 / complex128) vectors only, got %s' % dtype)


def _no_complex(t):
    if t is not None and t.is_complex():
        raise NotImplementedError('hmat: complex-valued matrices are not implemented (real matrices against real or '
                                  'complex vectors only)')


class _Builder:
    """collects the tiles of a tree in table order"""

    def __init__(self, dtype, device, require_cuda=True):
        self.dtype, self.device, self.require_cuda = dtype, device, require_cuda
        self.tiles, self.keep, self.scratch = [], [], 0

    def tensor(self, t, ndim):
        _no_complex(t)
        if self.require_cuda:
            _require_cuda(t)
        t = t.detach()
        if t.dtype != self.dtype or t.device != self.device:
            t = t.to(device=self.device, dtype=self.dtype)
        if ndim == 1 and not t.is_contiguous():
            t = t.contiguous()
        if ndim == 2 and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
            t = t.contiguous()
        self.keep.append(t)
        return t

    def add(self, a, ld, rows, cols, flags, stage, src_off, dst_off, scale, dst_scratch=False):
        if rows == 0 or (cols == 0 and not flags & DIAG):
            return
        self.tiles.append(dict(a=a.data_ptr(), ld=ld, rows=rows, cols=cols, flags=flags, stage=stage, src_off=src_off,
                               dst_off=dst_off, scale=scale, dst_scratch=dst_scratch))

    def dense(self, t, trans, src_off, dst_off, scale, stage=0, src_scratch=False, dst_scratch=False):
        t = self.tensor(t if t.ndim == 2 else t.reshape(len(t), -1), 2)
        flags = (TRANS if trans else 0) | (SRC_SCRATCH if src_scratch else 0)
        self.add(t, max(t.stride(0), t.shape[1]), t.shape[0], t.shape[1], flags, stage, src_off, dst_off, scale, dst_scratch)

    def diag(self, d, size, src_off, dst_off, scale, stage=0, scratch=False):
        d = self.tensor(d.reshape(-1), 1)
        if d.numel() not in (1, size):
            raise ValueError('hmat: a diagonal of %d elements for size %d' % (d.numel(), size))
        self.add(d, 1, size, 0 if (d.numel() == 1 and size > 1) else 1, DIAG | (SRC_SCRATCH if scratch else 0), stage, src_off,
                 dst_off, scale, scratch)

    def lowrank(self, left, left_t, right, right_t, src_off, dst_off, scale):
        """(left) (right) with left / right the stored tensors or, with *_t, their transposes.  The right factor has few
        outputs (the rank), and work is dealt by outputs: an input longer than SPLIT is cut into pieces whose partial products
        go to scratch segments of their own (stage 0, one work-group or more per piece), a unit diagonal tile per piece adds them
        in piece order into one segment (stage 1), and the left factor reads that segment (stage 2)."""
        right = self.tensor(right if right.ndim == 2 else right.reshape(len(right), -1), 2)
        rank, nin = (right.shape[1], right.shape[0]) if right_t else right.shape
        if rank == 0 or nin == 0:
            return
        pieces = min(-(-nin // SPLIT), MAX_PIECES)
        step = -(-(-(-nin // pieces)) // 16) * 16                  # a multiple of 16 elements: the pieces keep the alignment
        s = self.scratch
        if pieces == 1:
            self.scratch += rank
            self.dense(right, right_t, src_off, s, 1.0, stage=0, dst_scratch=True)
            self.dense(left, left_t, s, dst_off, scale, stage=1, src_scratch=True)
            return
        starts = list(range(0, nin, step))
        self.scratch += rank * (len(starts) + 1)
        total = s + rank * len(starts)
        for p, j in enumerate(starts):
            part = right[j:j + step] if right_t else right[:, j:j + step]
            self.dense(part, right_t, src_off + j, s + p * rank, 1.0, stage=0, dst_scratch=True)
        if not hasattr(self, 'one'):
            self.one = torch.ones(1, dtype=self.dtype, device=self.device)
        for p in range(len(starts)):
            self.diag(self.one, rank, s + p * rank, total, 1.0, stage=1, scratch=True)
        self.dense(left, left_t, total, dst_off, scale, stage=2, src_scratch=True)


def _emit(node, trans, r0, c0, scale, b):
    """the tiles of (node^T if trans else node) with its output at row r0 of y and its input at row c0 of x; False: not flattenable"""
    if isinstance(node, torch.Tensor):
        node = DenseMat(node)
    if isinstance(node, TransposedMat):
        return _emit(node._matobj, not trans, r0, c0, scale, b)
    if isinstance(node, DenseMat):
        b.dense(node.H, trans, c0, r0, scale)
    elif isinstance(node, DiagMat):
        b.diag(node.diag, node.size, c0, r0, scale)
    elif isinstance(node, TriangMat):
        b.dense(node.to_dense(), trans, c0, r0, scale)
    elif isinstance(node, ZeroMat):
        pass
    elif isinstance(node, SparseMat):
        U, V = node.U, node.V
        _no_complex(U)
        if not trans:
            b.lowrank(U, False, U if node.hermitian else V, node.hermitian, c0, r0, scale)
        else:
            b.lowrank(U if node.hermitian else V, not node.hermitian, U, True, c0, r0, scale)
        if node.Hdiag is not None:
            b.diag(node.Hdiag, len(node.Hdiag), c0, r0, scale)
    elif isinstance(node, (MatColumn, MatRow, PartitionedMat)) or type(node) is HierMat:
        if type(node) is HierMat and node.scalar is not None:
            scale = scale * float(node.scalar)
        for m, t, r, c in node._blocks(trans):
            if not _emit(m, t, r0 + r, c0 + c, scale, b):
                return False
    else:
        return False
    return True


def build_index(tiles, nout, scratch_rows):
    """
    The per-stage row ranges of a tile list (dicts as _Builder makes them): (ranges int64 [n, 5], tile_ids int32, stage_first).
    Stage 0 covers rows 0 ... nout - 1 of y in ranges of ROWS (a range without tiles writes zeros); a later stage holds the
    ranges of y that one of its tiles touches, flagged to accumulate.  The rows of the scratch vector are dealt per segment
    (the tiles of a stage that write the same rows): ROWS for a transposed or diagonal tile (its outputs run along the lanes),
    SCRATCH_ROWS for a plain one.
    """
    nstages = max([t['stage'] for t in tiles], default=0) + 1
    ranges, ids, stage_first = [], [], [0]

    def out_rows(t):
        return t['rows'] if t['flags'] & DIAG or not t['flags'] & TRANS else t['cols']

    def deal(flags, lo, hi, step, cand, keep_empty):
        for r in range(lo, hi, step):
            n = min(step, hi - r)
            hit = [i for i in cand if tiles[i]['dst_off'] < r + n and tiles[i]['dst_off'] + out_rows(tiles[i]) > r]
            if hit or keep_empty:
                ranges.append((flags, r, n, len(ids), len(hit)))
                ids.extend(hit)

    for s in range(nstages):
        mine = [i for i, t in enumerate(tiles) if t['stage'] == s]
        deal(ACCUMULATE if s else 0, 0, nout, ROWS, [i for i in mine if not tiles[i]['dst_scratch']], s == 0)
        segments = {}
        for i in mine:
            if tiles[i]['dst_scratch']:
                segments.setdefault((tiles[i]['dst_off'], out_rows(tiles[i])), []).append(i)
        for (off, n), group in segments.items():
            wide = any(tiles[i]['flags'] & (TRANS | DIAG) for i in group)
            deal(DST_SCRATCH, off, off + n, ROWS if wide else SCRATCH_ROWS, group, False)
        stage_first.append(len(ranges))
    return (np.asarray(ranges, dtype=np.int64).reshape(-1, 5), np.asarray(ids, dtype=np.int32), stage_first)


def pack_tiles(tiles):
    tab = np.zeros(len(tiles), dtype=TILE_DTYPE)
    for i, t in enumerate(tiles):
        for k in ('a', 'ld', 'src_off', 'dst_off', 'scale', 'rows', 'cols', 'flags', 'stage'):
            tab[k][i] = t[k]
    return tab


class Plan:
    """the flattened form of one operator (or its transpose) for one dtype and device"""

    def __init__(self, node, dtype, device, transpose):
        b = _Builder(dtype, device)
        self.ok = _emit(node, transpose, 0, 0, 1.0, b)
        self.epoch = _EPOCH[0]
        if not self.ok:
            return
        shape = tuple(node.shape)
        self.nout, self.nin = (shape[1], shape[0]) if transpose else shape
        self.dtype, self.device, self.code = dtype, device, _code(dtype)
        self.tiles, self.keep, self.scratch_rows = b.tiles, b.keep, b.scratch
        self.table = pack_tiles(b.tiles)
        self.ranges, self.ids, self.stage_first = build_index(b.tiles, self.nout, b.scratch)
        self.nstages = len(self.stage_first) - 1
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device)
        self.table_dev, self.ranges_dev, self.ids_dev = put(self.table), put(self.ranges), put(self.ids)
        self.stage_first_c = (ctypes.c_int * len(self.stage_first))(*self.stage_first)
        self.ws = None

    def apply(self, x, y, nrhs, scalar=1.0, accumulate=False):
        """y (+)= scalar * A x for contiguous real x [nin, nrhs], y [nout, nrhs] on the plan's device"""
        need = int(_lib.lib.rime_hmat_workspace(self.code, self.scratch_rows, nrhs))
        if need and (self.ws is None or self.ws.numel() < need):
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.rime_hmat_apply(self.code, _ptr(self.table_dev), len(self.tiles), _ptr(self.ranges_dev),
                                                _ptr(self.ids_dev), self.stage_first_c, self.nstages, self.scratch_rows, _ptr(x),
                                                _ptr(y), nrhs, float(scalar), int(bool(accumulate)),
                                                _ptr(self.ws if need else None), need, _stream()), 'rime_hmat_apply')


def _plan(node, dtype, device, transpose):
    plans = node.__dict__.setdefault('_plans', {})
    key = (dtype, torch.device(device), bool(transpose))
    p = plans.get(key)
    if p is None or p.epoch != _EPOCH[0]:
        p = plans[key] = Plan(node, dtype, torch.device(device), bool(transpose))
    return p if p.ok else None


def _add_out(result, out):
    if out is None:
        return result
    out[:] += result
    return out


def _apply(node, vec, transpose=False, out=None, scalar=None):
    """(scalar *) node (or its transpose) times vec [N] or [N, M], real or complex, through the plan; out[:] += result"""
    _require_cuda(vec, out)
    plan = _plan(node, _real(vec.dtype), vec.device, transpose)
    if plan is None:
        res = node._leafwise(vec, transpose)
        return _add_out(res if scalar is None else res * scalar, out)
    if vec.shape[0] != plan.nin:
        raise ValueError('hmat: a vector of %d rows for an operator of %d columns' % (vec.shape[0], plan.nin))
    x = vec.detach().resolve_conj().contiguous()
    shape = (plan.nout,) + tuple(vec.shape[1:])
    direct = (out is not None and out.is_contiguous() and out.dtype == vec.dtype and tuple(out.shape) == shape
              and out.device == vec.device and not out.is_conj())
    y = out if direct else torch.empty(shape, dtype=vec.dtype, device=vec.device)
    nrhs = (x.numel() // max(plan.nin, 1)) * (2 if vec.is_complex() else 1)
    if plan.nout and nrhs:
        if plan.nin == 0:
            if not direct:
                y.zero_()
        else:
            rv = lambda t: torch.view_as_real(t) if t.is_complex() else t
            plan.apply(rv(x), rv(y.detach()), nrhs, 1.0 if scalar is None else scalar, accumulate=direct)
    return y if direct else _add_out(y, out)


class BaseMat(object):
    """what the operators share: products through the plan, call, transposed view, invalidation"""

    @property
    def shape(self):
        return self._shape

    def mat_vec_mul(self, vec, transpose=False, out=None, **kwargs):
        return _apply(self, vec, transpose, out)

    def mat_mat_mul(self, mat, transpose=False, out=None, **kwargs):
        return _apply(self, mat, transpose, out)

    def __call__(self, vec, **kwargs):
        return self.mat_vec_mul(vec, **kwargs) if vec.ndim == 1 else self.mat_mat_mul(vec, **kwargs)

    def _leafwise(self, vec, transpose):
        raise NotImplementedError('%s has no product outside the plan' % type(self).__name__)

    def to_transpose(self):
        return TransposedMat(self)

    def to_dense(self, transpose=False):
        raise NotImplementedError

    def diagonal(self):
        return self.to_dense().diagonal()

    def least_squares(self, y, **kwargs):
        return linalg.least_squares(self.to_dense(), y, **kwargs)

    def __rmul__(self, other):
        return self.__mul__(other)

    def __imul__(self, other):
        self.scalar_mul(other)
        return self

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_plans', None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        _touch()

    def __str__(self):
        return "<{} ({}x{})>".format(self.__class__.__name__, *self.shape)


def _ct(H, transpose):
    return H.T.conj() if transpose and H.is_complex() else (H.T if transpose else H)


class DenseMat(BaseMat):
    """a dense rectangular matrix"""

    def __init__(self, H):
        if H.ndim == 1:
            H = H[:, None]
        self._set(H)

    def _set(self, H):
        self.H, self._shape = H, tuple(H.shape)
        self._complex, self.dtype, self.device = torch.is_complex(H), H.dtype, H.device

    def to_dense(self, transpose=False):
        return _ct(self.H, transpose)

    def push(self, device):
        self._set(utils.push(self.H, device))
        _touch(self)

    def scalar_mul(self, scalar):
        self.H *= scalar
        _touch(self)

    def diagonal(self):
        return self.H.diagonal()

    def least_squares(self, y, **kwargs):
        return linalg.least_squares(self.H, y, **kwargs)

    def __mul__(self, other):
        return DenseMat(self.H * other)


class DiagMat(BaseMat):
    """a diagonal matrix, or a scalar one: a single value and size >= 1"""

    def __init__(self, diag, size=None):
        self.diag = diag
        self.size = size if size is not None else diag.numel()
        self._complex, self.dtype, self.device = torch.is_complex(diag), diag.dtype, diag.device

    @property
    def shape(self):
        return (self.size, self.size)

    def to_dense(self, transpose=False, **kwargs):
        return torch.diag(self.diagonal().conj() if transpose and self._complex else self.diagonal())

    def push(self, device):
        self.diag = utils.push(self.diag, device)
        self.dtype, self.device = self.diag.dtype, self.diag.device
        _touch(self)

    def scalar_mul(self, scalar):
        self.diag *= scalar
        _touch(self)

    def diagonal(self):
        return torch.atleast_1d(self.diag).expand((self.size,))

    def least_squares(self, y, **kwargs):
        return DiagMat(1 / self.diag, self.size)(y)

    def __mul__(self, other):
        return DiagMat(self.diag * other, self.size)


class HadamardMat(BaseMat):
    """an n-dimensional array multiplied element by element into its argument (a torch expression, outside the plan)"""

    _set = DenseMat._set

    def __init__(self, H):
        self._set(H)

    def mat_vec_mul(self, vec, transpose=False, out=None, **kwargs):
        return self.mat_mat_mul(vec, transpose=transpose, out=out, **kwargs)

    def mat_mat_mul(self, mat, transpose=False, out=None, square=False, **kwargs):
        _require_cuda(mat, out)
        H = _ct(self.H, transpose)
        return _add_out((H ** 2 if square else H) * mat, out)

    def __call__(self, mat, **kwargs):
        return self.mat_mat_mul(mat, **kwargs)

    def _leafwise(self, vec, transpose):
        return self.mat_mat_mul(vec, transpose=transpose)

    def to_dense(self, transpose=False):
        return _ct(self.H, transpose)

    push, scalar_mul = DenseMat.push, DenseMat.scalar_mul

    def diagonal(self):
        return self.H if self.H.ndim == 1 else self.H.diagonal()

    def least_squares(self, y, **kwargs):
        return HadamardMat(1 / self.H)(y)

    def __mul__(self, other):
        return HadamardMat(self.H * other)


class TriangMat(BaseMat):
    """a square triangular matrix of which only the triangle is stored"""

    def __init__(self, L, lower=True):
        self.device = L.device
        if L.ndim == 1:
            n = int(round((np.sqrt(8 * len(L) + 1) - 1) / 2))
            shape = (n, n)
        else:
            shape = tuple(L.shape)
        self.idx = (torch.tril_indices if lower else torch.triu_indices)(*shape, device=self.device)
        if L.ndim == 2:
            L = L[self.idx[0], self.idx[1]]
        self.L, self.dtype, self.lower, self._shape = L, L.dtype, lower, shape
        self._diag_idx = torch.where(self.idx[0] == self.idx[1])[0]
        self._complex = torch.is_complex(L)

    def to_dense(self, transpose=False):
        H = torch.zeros(self.shape, device=self.device, dtype=self.dtype)
        H[self.idx[0], self.idx[1]] = self.L
        return _ct(H, transpose)

    def push(self, device):
        self.L = utils.push(self.L, device)
        if not isinstance(device, torch.dtype):
            self.idx, self._diag_idx = utils.push(self.idx, device), utils.push(self._diag_idx, device)
        self.dtype, self.device = self.L.dtype, self.L.device
        _touch(self)

    def scalar_mul(self, scalar):
        self.L *= scalar
        _touch(self)

    def diagonal(self):
        return self.L[self._diag_idx]

    def __mul__(self, other):
        return TriangMat(self.L * other, lower=self.lower)


class SparseMat(BaseMat):
    """diagonal plus low rank: M = diag(Hdiag) + U V, U (Nrows, Nmodes), V (Nmodes, Ncols) or, hermitian, V = U^H"""

    def __init__(self, shape, U, V=None, Hdiag=None, hermitian=False):
        self._shape, self.Hdiag, self.U = tuple(shape), Hdiag, U
        self._complex, self.device, self.dtype = torch.is_complex(U), U.device, U.dtype
        self.V = None if hermitian else V
        self.hermitian = hermitian

    def _V(self):
        return self.U.T.conj() if self.hermitian and self._complex else (self.U.T if self.hermitian else self.V)

    def to_dense(self, transpose=False):
        out = self.U @ self._V()
        if self.Hdiag is not None:
            out.diagonal()[:len(self.Hdiag)] += self.Hdiag
        return _ct(out, transpose)

    def push(self, device):
        self.U, self.V, self.Hdiag = utils.push(self.U, device), utils.push(self.V, device), utils.push(self.Hdiag, device)
        self._complex, self.dtype, self.device = torch.is_complex(self.U), self.U.dtype, self.U.device
        _touch(self)

    def scalar_mul(self, scalar):
        self.U *= scalar
        if self.Hdiag is not None:
            self.Hdiag *= scalar
        _touch(self)

    def diagonal(self):
        N = min(self._shape)
        diag = (self.U[:N] * self._V().T[:N]).sum(1)
        if self.Hdiag is not None:
            diag[:len(self.Hdiag)] += self.Hdiag
        return diag

    def least_squares(self, y, **kwargs):
        """Woodbury: (A + U V)^-1 = A^-1 - A^-1 U (I + V A^-1 U)^-1 V A^-1 with A = diag(Hdiag)"""
        Ainv = 1 / self.Hdiag
        U, V = self.U, self._V()
        inner = torch.linalg.pinv(torch.eye(len(V), dtype=U.dtype, device=U.device) + (V * Ainv) @ U)
        ya = Ainv * y if y.ndim == 1 else Ainv[:, None] * y
        t = U @ (inner @ (V @ ya))
        return ya - (Ainv * t if y.ndim == 1 else Ainv[:, None] * t)

    def __mul__(self, other):
        U, V = self.U, self.V
        if V is not None:
            V = V * other
        else:
            U = other[:, None] * U if isinstance(other, torch.Tensor) and other.ndim else U * other
        return SparseMat(self.shape, U, V=V, Hdiag=None if self.Hdiag is None else self.Hdiag * other, hermitian=self.hermitian)

    def __rmul__(self, other):
        U = other[:, None] * self.U if isinstance(other, torch.Tensor) and other.ndim else self.U * other
        return SparseMat(self.shape, U, V=self.V, Hdiag=None if self.Hdiag is None else self.Hdiag * other,
                         hermitian=self.hermitian)


class ZeroMat(BaseMat):
    """a matrix of zeros (no tile in a plan)"""

    def __init__(self, shape, dtype=None, device=None):
        self._shape = tuple(shape)
        self.dtype = dtype if dtype is not None else utils._float()
        self.device = device

    def to_dense(self, transpose=False):
        return torch.zeros(self.shape[::-1] if transpose else self.shape, dtype=self.dtype, device=self.device)

    def push(self, device):
        if isinstance(device, torch.dtype):
            self.dtype = device
        else:
            self.device = device
        _touch(self)

    def scalar_mul(self, scalar):
        pass

    def diagonal(self):
        return torch.zeros(min(self._shape), dtype=self.dtype, device=self.device)

    def __mul__(self, other):
        return ZeroMat(self.shape, device=self.device, dtype=self.dtype)

    def __imul__(self, other):
        return self


class OneMat(BaseMat):
    """every element equal to `scalar` (rank one; a torch expression, outside the plan)"""

    def __init__(self, shape, scalar=1.0, dtype=None, device=None):
        self._shape, self.scalar = tuple(shape), scalar
        self.dtype = dtype if dtype is not None else utils._float()
        self.device = device

    def mat_vec_mul(self, vec, transpose=False, out=None, **kwargs):
        _require_cuda(vec, out)
        n = self.shape[1] if transpose else self.shape[0]
        total = vec.sum(dim=0, keepdim=True) * self.scalar
        return _add_out(total.expand((n,) + tuple(vec.shape[1:])).clone(), out)

    mat_mat_mul = mat_vec_mul

    def _leafwise(self, vec, transpose):
        return self.mat_vec_mul(vec, transpose=transpose)

    def to_dense(self, transpose=False):
        return torch.ones(self.shape[::-1] if transpose else self.shape, dtype=self.dtype, device=self.device) * self.scalar

    push = ZeroMat.push

    def scalar_mul(self, scalar):
        self.scalar *= scalar
        _touch(self)

    def diagonal(self):
        return torch.ones(min(self._shape), dtype=self.dtype, device=self.device) * self.scalar

    def __mul__(self, other):
        other = other.scalar if isinstance(other, OneMat) else other
        return OneMat(self.shape, self.scalar * other, device=self.device, dtype=self.dtype)

    def __imul__(self, other):
        return self * other


class TransposedMat(BaseMat):
    """a view of an operator as its (conjugate) transpose; no data is copied"""

    def __init__(self, matobj):
        if isinstance(matobj, torch.Tensor):
            matobj = DenseMat(matobj)
        self._matobj, self.dtype, self.device = matobj, matobj.dtype, matobj.device

    @property
    def shape(self):
        return tuple(self._matobj.shape[::-1])

    def _leafwise(self, vec, transpose):
        return self._matobj.mat_vec_mul(vec, transpose=not transpose)

    def to_dense(self, transpose=False):
        return self._matobj.to_dense(transpose=not transpose)

    def push(self, device):
        self._matobj.push(device)
        self.dtype, self.device = self._matobj.dtype, self._matobj.device
        _touch(self)

    def __repr__(self):
        return "<TransposedMat({})>".format(str(self._matobj))

    def scalar_mul(self, scalar):
        scalar = torch.as_tensor(scalar)
        self._matobj.scalar_mul(scalar.conj() if scalar.is_complex() else scalar)
        _touch(self)

    def diagonal(self):
        return self._matobj.diagonal()

    def __mul__(self, other):
        return TransposedMat(self._matobj * other)

    def __rmul__(self, other):
        return TransposedMat(other * self._matobj)


class _BlockMat(BaseMat):
    """an operator assembled from blocks: _blocks(transpose) lists (block, its transpose flag, first row, first column)"""

    def _leaves(self):
        seen, out = set(), []
        for m, _, _, _ in self._blocks(False):
            while isinstance(m, TransposedMat):
                m = m._matobj
            if id(m) not in seen:
                seen.add(id(m))
                out.append(m)
        return out

    def _leafwise(self, vec, transpose):
        n = self.shape[1] if transpose else self.shape[0]
        res = torch.zeros((n,) + tuple(vec.shape[1:]), dtype=vec.dtype, device=vec.device)
        for m, t, r, c in self._blocks(transpose):
            nr, nc = m.shape[::-1] if t else m.shape
            res[r:r + nr] += m.mat_vec_mul(vec[c:c + nc], transpose=t)
        return res

    def to_dense(self, transpose=False, **kwargs):
        blocks = self._blocks(transpose)
        first = blocks[0][0].to_dense()
        out = torch.zeros(self.shape[::-1] if transpose else self.shape, dtype=first.dtype, device=first.device)
        for m, t, r, c in blocks:
            d = m.to_dense(transpose=t)
            out[r:r + d.shape[0], c:c + d.shape[1]] = d
        return out

    def push(self, device):
        for m in self._leaves():
            m.push(device)
        _touch(self)

    def scalar_mul(self, scalar):
        for m in self._leaves():
            m.scalar_mul(scalar)
        _touch(self)


class PartitionedMat(_BlockMat):
    """
    A matrix partitioned into on-diagonal blocks (keys (i, i)) and off-diagonal blocks (keys (i, j)) of a dictionary.  A
    missing off-diagonal block is zero; with symmetric=True only one of (i, j), (j, i) is given and the other is its
    transpose.  The blocks are held as one MatColumn per column of blocks (matcols), with vec_idx the slices of the input.
    """

    def __init__(self, blocks, symmetric=True):
        for k, v in blocks.items():
            if isinstance(v, torch.Tensor):
                blocks[k] = DiagMat(v, len(v)) if v.ndim == 1 else DenseMat(v)
        keys = sorted(k for k in blocks if k[0] == k[1])
        self._Ncols = len(keys)
        self._shape = (sum(blocks[k].shape[0] for k in keys), sum(blocks[k].shape[1] for k in keys))
        self.dtype, self.device, self.symmetric = blocks[keys[0]].dtype, blocks[keys[0]].device, symmetric
        self.matcols, self.diagmats, self.vec_idx = [], [], []
        col = 0
        for k in keys:
            self.diagmats.append(blocks[k])
            self.vec_idx.append(slice(col, col + blocks[k].shape[1]))
            col += blocks[k].shape[1]
            mats = []
            for j in keys:
                bk = (j[0], k[1])
                if bk in blocks:
                    mats.append(blocks[bk])
                elif symmetric and bk[::-1] in blocks:
                    mats.append(TransposedMat(blocks[bk[::-1]]))
                else:
                    blocks[bk] = ZeroMat((blocks[j].shape[0], blocks[k].shape[1]), dtype=self.dtype, device=self.device)
                    mats.append(blocks[bk])
            self.matcols.append(MatColumn(mats))

    def _blocks(self, transpose):
        out = []
        for mc, idx in zip(self.matcols, self.vec_idx):
            out.extend((m, t, r + idx.start, c) if transpose else (m, t, r, c + idx.start) for m, t, r, c in mc._blocks(transpose))
        return out

    def to_transpose(self):
        return PartitionedMat({(i + 1, j + 1): TransposedMat(m) for i, mc in enumerate(self.matcols) for j, m in enumerate(mc.mats)},
                              symmetric=self.symmetric)

    def push(self, device):
        _BlockMat.push(self, device)
        self.dtype, self.device = self.matcols[0].mats[0].dtype, self.matcols[0].mats[0].device

    def diagonal(self):
        return torch.cat([b.diagonal() for b in self.diagmats])

    def least_squares(self, y, **kwargs):
        """block-diagonal solve only, as in the reference"""
        return torch.cat([m.least_squares(y[idx], **kwargs) for idx, m in zip(self.vec_idx, self.diagmats)])

    def _scaled(self, f):
        return PartitionedMat({(j + 1, i + 1): f(m) for i, mc in enumerate(self.matcols) for j, m in enumerate(mc.mats)},
                              symmetric=self.symmetric)

    def __mul__(self, other):
        return self._scaled(lambda m: m * other)

    def __rmul__(self, other):
        return self._scaled(lambda m: other * m)


class MatColumn(_BlockMat):
    """operators of equal Ncols stacked vertically"""
    _axis = 0

    def __init__(self, mats):
        self.mats = mats
        self.idx, n, other = [], 0, self.mats[0].shape[1 - self._axis]
        for m in self.mats:
            assert other == m.shape[1 - self._axis]
            self.idx.append(slice(n, n + m.shape[self._axis]))
            n += m.shape[self._axis]
        self._shape = (n, other) if self._axis == 0 else (other, n)
        self.dtype, self.device = mats[0].dtype, mats[0].device

    def _blocks(self, transpose):
        along_rows = (self._axis == 0) != bool(transpose)
        return [(m, bool(transpose), s.start, 0) if along_rows else (m, bool(transpose), 0, s.start) for m, s in zip(self.mats, self.idx)]

    def __repr__(self):
        return "<{} of shape {}>".format(type(self).__name__, self.shape)

    def to_transpose(self):
        return (MatRow if self._axis == 0 else MatColumn)([TransposedMat(m) for m in self.mats])

    def __mul__(self, other):
        return type(self)([m * other for m in self.mats])

    def __rmul__(self, other):
        return type(self)([other * m for m in self.mats])


class MatRow(MatColumn):
    """operators of equal Nrows side by side"""
    _axis = 1


class MatSum:
    """operators of one shape whose products are added"""

    def __init__(self, mats):
        self.mats = mats

    def mat_vec_mult(self, vec, **kwargs):
        return sum(m(vec, **kwargs) for m in self.mats)

    mat_vec_mul = mat_vec_mult

    def __call__(self, vec, **kwargs):
        return self.mat_vec_mult(vec, **kwargs)

    def to_dense(self, sum=True, transpose=False):
        out = torch.stack([m.to_dense(transpose=transpose) for m in self.mats])
        return out.sum(0) if sum else out

    def push(self, device):
        for m in self.mats:
            m.push(device)

    def scalar_mul(self, scalar):
        for m in self.mats:
            m.scalar_mul(scalar)

    def __mul__(self, other):
        return MatSum([m * other for m in self.mats])

    def __rmul__(self, other):
        return MatSum([other * m for m in self.mats])

    def __imul__(self, other):
        self.scalar_mul(other)
        return self


class MatDict:
    """operators under string keys, the mirror of ParamDict"""

    def __init__(self, mats):
        self.mats = mats
        self._setup()

    def _setup(self):
        self.devices = {k: self.mats[k].device for k in self.keys()}

    def keys(self):
        return list(self.mats.keys())

    def values(self):
        return list(self.mats.values())

    def items(self):
        return list(self.mats.items())

    def push(self, device):
        for k in (device if isinstance(device, dict) else self.mats):
            self.mats[k].push(device[k] if isinstance(device, dict) else device)
        self._setup()
        _touch()

    def to_dense(self, transpose=False):
        return paramdict.ParamDict({k: self.mats[k].to_dense(transpose=transpose) for k in self.keys()})

    def mat_vec_mul(self, vec, **kwargs):
        out = {}
        for k in self.keys():
            if k in vec:
                o = self.mats[k].mat_vec_mul(vec[k].reshape(-1), **kwargs)
                out[k] = o.reshape(vec[k].shape)
        return paramdict.ParamDict(out)

    def __getitem__(self, key):
        return self.mats[key]

    def __setitem__(self, key, val):
        self.mats[key] = val
        _touch()

    def update(self, other):
        for key in other:
            self[key] = other[key]
        self._setup()

    def __iter__(self):
        return (p for p in self.mats)


class HierMat(_BlockMat):
    """
    A 2 x 2 block matrix whose blocks may be HierMat again (HODLR): H[0] or H[(0, 0)], H[1] or H[(1, 1)], H[(0, 1)], H[(1, 0)].
    A missing off-diagonal block is zero; with sym the missing one is the transpose of the other.  `scalar` multiplies the product.
    """

    def __init__(self, A00, A11, A01=None, A10=None, sym=False, scalar=None):
        A00, A11, A01, A10 = [DenseMat(a) if isinstance(a, torch.Tensor) else a for a in (A00, A11, A01, A10)]
        if sym:
            if A01 is None and A10 is not None:
                A01 = TransposedMat(A10)
            if A10 is None and A01 is not None:
                A10 = TransposedMat(A01)
        self.A00, self.A11, self.A01, self.A10 = A00, A11, A01, A10
        if A01 is not None:
            assert A01.shape[0] == A00.shape[0] and A01.shape[1] == A11.shape[1]
        if A10 is not None:
            assert A10.shape[0] == A11.shape[0] and A10.shape[1] == A00.shape[1]
        self.dtype, self.device, self.sym, self.scalar = A00.dtype, A00.device, sym, scalar
        self._shape0, self._shape1 = tuple(A00.shape), tuple(A11.shape)
        self._shape = (A00.shape[0] + A11.shape[0], A00.shape[1] + A11.shape[1])
        self._idx0 = (slice(self._shape0[0]), slice(self._shape0[1]))
        self._idx1 = (slice(self._shape0[0], self._shape[0]), slice(self._shape0[1], self._shape[1]))

    def _blocks(self, transpose):
        R, C = self._shape0
        out = [(self.A00, bool(transpose), 0, 0)]
        if self.A10 is not None:
            out.append((self.A10, True, 0, R) if transpose else (self.A10, False, R, 0))
        out.append((self.A11, True, C, R) if transpose else (self.A11, False, R, C))
        if self.A01 is not None:
            out.append((self.A01, True, C, 0) if transpose else (self.A01, False, 0, C))
        return out

    def _leafwise(self, vec, transpose):
        res = _BlockMat._leafwise(self, vec, transpose)
        return res if self.scalar is None else res * self.scalar

    def diagonal(self, return_tensor=True):
        diag = []
        for a in (self.A00, self.A11):
            diag.extend(a.diagonal(False) if isinstance(a, HierMat) else [a.diagonal()])
        if self.scalar is not None:
            diag = [d * self.scalar for d in diag]
        return torch.cat(diag) if return_tensor else diag

    def __getitem__(self, idx):
        return {0: self.A00, (0, 0): self.A00, 1: self.A11, (1, 1): self.A11, (0, 1): self.A01, (1, 0): self.A10}.get(idx)

    def push(self, device):
        self.scalar = utils.push(self.scalar, device) if isinstance(self.scalar, torch.Tensor) else self.scalar
        for a in (self.A00, self.A11, self.A01, self.A10):
            if a is not None:
                a.push(device)
        self.device = self.A00.device
        _touch(self)

    def to_transpose(self):
        t = lambda a: None if a is None else a.to_transpose()
        return HierMat(A00=t(self.A00), A11=t(self.A11), A10=t(self.A01), A01=t(self.A10), sym=self.sym, scalar=self.scalar)

    def to_dense(self, transpose=False):
        H = _BlockMat.to_dense(self, transpose)
        return H if self.scalar is None else H * self.scalar

    def scalar_mul(self, scalar):
        if self.scalar is None:
            self.scalar = torch.tensor(1.0, device=self.device)
        self.scalar = self.scalar * scalar
        _touch(self)

    def to_SolveHierMat(self, lower=True, trans_solve=False):
        """self as the Cholesky factor of a SolveHierMat (a new object)"""
        scalar = 1 / self.scalar if self.scalar is not None else None
        if scalar is not None and trans_solve:
            scalar = scalar ** 2
        return SolveHierMat(self.A00, self.A11, A01=self.A01, A10=self.A10, lower=lower, trans_solve=trans_solve, scalar=scalar)

    def least_squares(self, y, **kwargs):
        if self.A10 is None and self.A01 is None:
            return torch.cat([self.A00.least_squares(y[self._idx0[1]], **kwargs), self.A11.least_squares(y[self._idx1[1]], **kwargs)])
        return torch.linalg.lstsq(self.to_dense(), y)

    def __mul__(self, other):
        raise NotImplementedError('HierMat has no out-of-place product with a scalar; use scalar_mul')

    def __repr__(self):
        return "{}\n| {}, {} |\n| {}, {} |".format(self, self.A00, self.A01, self.A10, self.A11)


def _split_solve(fn, A, B, **kwargs):
    """fn(A, B) with a complex B against a real A as ONE solve of [Re B, Im B]"""
    if torch.is_complex(B) and not torch.is_complex(A):
        rB = B[:, None] if B.ndim == 1 else B
        n = rB.shape[1]
        out = fn(A, torch.cat([rB.real, rB.imag], dim=-1), **kwargs)
        out = torch.complex(out[:, :n], out[:, n:])
        return out[:, 0] if B.ndim == 1 else out
    return fn(A, B, **kwargs)


class SolveMat(BaseMat):
    """
    The inverse of A as an operator: the product with b is the solution x of A x = b, by substitution for a triangular A
    (tri), by a general solve otherwise; with chol, A is a triangular Cholesky factor and the system is A A^H x = b.  A 1-D
    A is a diagonal.  Sequential by nature: torch.linalg.solve_triangular / solve.
    """

    def __init__(self, A, tri=False, lower=True, chol=False):
        if isinstance(A, DiagMat):
            A = A.diagonal()
        if isinstance(A, BaseMat):
            A = A.to_dense()
        self.A = A
        self._shape = (len(A), len(A)) if A.ndim == 1 else tuple(A.shape)
        self.device, self.dtype, self.tri, self.lower, self.chol = A.device, A.dtype, tri, lower, chol
        if chol:
            assert self.tri, "If passing A as chol, it must also be triangular"

    def mat_vec_mul(self, vec, transpose=False, out=None, chol=None, **kwargs):
        _require_cuda(vec, out, self.A)
        chol = self.chol if chol is None else chol
        A = _ct(self.A, transpose) if self.A.ndim == 2 else self.A
        lower = self.lower != bool(transpose)
        if A.ndim == 1:
            result = vec / (A if vec.ndim == 1 else A[:, None])
        elif self.tri:
            b = vec[:, None] if vec.ndim == 1 else vec
            result = self._solve_tri(A, b, upper=not lower)
            if chol:
                result = self._solve_tri(_ct(A, True), result, upper=lower)
            if vec.ndim == 1:
                result = result[:, 0]
        else:
            result = self._solve(A, vec)
        return _add_out(result, out)

    mat_mat_mul = mat_vec_mul

    def __call__(self, vec, **kwargs):
        return self.mat_vec_mul(vec, **kwargs)

    def _leafwise(self, vec, transpose):
        return self.mat_vec_mul(vec, transpose=transpose)

    def _solve_tri(self, A, B, upper=False, **kwargs):
        return _split_solve(torch.linalg.solve_triangular, A, B, upper=upper, **kwargs)

    def _solve(self, A, B, **kwargs):
        return _split_solve(torch.linalg.solve, A, B, **kwargs)

    def push(self, device):
        self.A = utils.push(self.A, device)
        self.device, self.dtype = self.A.device, self.A.dtype
        _touch(self)

    def to_dense(self, **kwargs):
        return self(torch.eye(self.shape[1], device=self.device, dtype=self.dtype), **kwargs)

    def to_transpose(self):
        if self.tri:
            return SolveMat(_ct(self.A, True), tri=self.tri, lower=not self.lower, chol=self.chol)
        return TransposedMat(self)

    def scalar_mul(self, scalar):
        self.A /= scalar
        _touch(self)

    def diagonal(self):
        if self.chol:
            q = torch.randn(self.shape[0], 3000, device=self.device, dtype=self.dtype)
            return self(q, transpose=True, chol=False).var(1)
        return self.to_dense().diagonal()

    def __mul__(self, other):
        return SolveMat(self.A / other, tri=self.tri, lower=self.lower, chol=self.chol)


class SolveHierMat(HierMat):
    """
    A HierMat of a triangular (Cholesky) factor applied as a solve: given lower-triangular L, the product with x is z of
    L z = x by block substitution; the on-diagonal blocks are SolveMat or SolveHierMat, the off-diagonal block any operator
    (its product goes through its plan).  trans_solve adds the solve against the transpose: L L^T z = x.
    """

    def __init__(self, A00, A11, A01=None, A10=None, lower=True, trans_solve=False, scalar=None):
        def solver(a):
            if a.__class__ == HierMat:
                return a.to_SolveHierMat(lower=lower, trans_solve=False)
            if isinstance(a, BaseMat) and not isinstance(a, SolveMat):
                a = a.diagonal() if isinstance(a, DiagMat) else a.to_dense()
            return SolveMat(a, tri=True, lower=lower, chol=False) if isinstance(a, torch.Tensor) else a

        super().__init__(solver(A00), solver(A11), A01, A10, sym=False, scalar=scalar)
        self.lower, self.trans_solve, self._T = lower, trans_solve, None

    def mat_vec_mul(self, vec, out=None, transpose=False, trans_solve=None, **kwargs):
        _require_cuda(vec, out)
        if transpose:
            self = self.to_transpose()
        i0, i1 = self._idx0[1], self._idx1[1]
        if self.lower:
            z0 = self[0](vec[i0], trans_solve=False)
            v1 = vec[i1] if self[(1, 0)] is None else vec[i1] - self[(1, 0)](z0)
            z1 = self[1](v1, trans_solve=False)
        else:
            z1 = self[1](vec[i1], trans_solve=False)
            v0 = vec[i0] if self[(0, 1)] is None else vec[i0] - self[(0, 1)](z1)
            z0 = self[0](v0, trans_solve=False)
        res = torch.cat([z0, z1])
        if self.scalar is not None:
            res = res * self.scalar
        if self.trans_solve if trans_solve is None else trans_solve:
            res = self.to_transpose()(res, trans_solve=False)
        return _add_out(res, out)

    mat_mat_mul = mat_vec_mul

    def __call__(self, vec, **kwargs):
        return self.mat_vec_mul(vec, **kwargs)

    def _leafwise(self, vec, transpose):
        return self.mat_vec_mul(vec, transpose=transpose)

    def to_dense(self, transpose=False, **kwargs):
        return self(torch.eye(self.shape[1], device=self.device, dtype=self.dtype), transpose=transpose, **kwargs)

    def diagonal(self, return_tensor=True):
        return self.to_dense().diagonal()

    def to_transpose(self):
        if self._T is None:
            t = lambda a: None if a is None else a.to_transpose()
            self._T = SolveHierMat(A00=t(self.A00), A11=t(self.A11), A10=t(self.A01), A01=t(self.A10), lower=not self.lower,
                                   scalar=self.scalar, trans_solve=self.trans_solve)
        return self._T

    def push(self, device):
        HierMat.push(self, device)
        self._T = None

    def scalar_mul(self, scalar):
        HierMat.scalar_mul(self, scalar)
        if self._T is not None:
            self._T.scalar_mul(scalar)


def make_hodlr(mat, indices, trisolve=False, lower=True, Nrank=None, rcond=None, sparse_tol=None):
    """construct a hierarchical (HODLR) matrix: not implemented, as in the reference"""
    raise NotImplementedError
