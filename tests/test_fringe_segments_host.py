"""
The block -> (segment, f, t, split) map of a merged pair launch (seg_plan / seg_block, csrc/fringe_mfma_common.h, through
rime_fringe_pair_segments_map): every block index of the shapes of tests/test_fringe_segments_gpu.py and of the C4 step is
enumerated; each (segment, f, t, split) occurs exactly once, the panel / tile ranges tile every segment, the segment with
the most pixels stands first in the grid, and one segment is the plan of the single launch.  No GPU.
"""
import ctypes

import numpy as np
import pytest

import fringe_kernel_table as kt
from test_pair_bwd_split_host import pair_bwd_splits

# (Nt, Nf, padded pixels per segment)
SHAPES = [
    (2, 3, (128, 64)), (2, 3, (64, 64, 128)), (2, 3, (16448, 64)), (2, 3, (128, 2112)), (2, 3, (64,)), (1, 1, (64, 64, 64, 64)),
    (8, 256, (98304, 10048)), (8, 256, (10048, 98304)), (8, 256, (98304,)), (8, 256, (10048,)),
]


def block_map(backward, Nt, Nf, Ps):
    from bayeslim_amd import ops
    f = ops.lib.rime_fringe_pair_segments_map
    arr = (ctypes.c_int * len(Ps))(*Ps)
    n = f(int(backward), Nt, Nf, arr, len(Ps), None, 0)
    assert n > 0
    out = np.zeros((n, 6), dtype=np.int32)
    assert f(int(backward), Nt, Nf, arr, len(Ps), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n) == n
    assert f(int(backward), Nt, Nf, arr, len(Ps), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n - 1) == -2
    return out


@pytest.mark.parametrize('backward', [False, True])
@pytest.mark.parametrize('Nt,Nf,Ps', SHAPES)
def test_every_block_once_and_ranges_tile_the_segments(backward, Nt, Nf, Ps):
    m = block_map(backward, Nt, Nf, Ps)
    seg, f, t, split, beg, end = m.T
    assert len({tuple(r[:4]) for r in m.tolist()}) == len(m), 'a (segment, f, t, split) occurs twice'
    assert (beg < end).all()
    for k, P in enumerate(Ps):
        rows = m[seg == k]
        S = rows[:, 3].max() + 1
        assert len(rows) == Nt * Nf * S
        assert set(map(tuple, rows[:, 1:4].tolist())) == {(a, b, c) for a in range(Nf) for b in range(Nt) for c in range(S)}
        one = rows[(rows[:, 1] == 0) & (rows[:, 2] == 0)]
        one = one[np.argsort(one[:, 3])]
        assert one[0, 4] == 0 and one[-1, 5] == P // 32 and (one[1:, 4] == one[:-1, 5]).all(), 'ranges do not tile segment %d' % k
        # every (f, t) of a split has the split's range
        for r in one:
            assert (rows[rows[:, 3] == r[3]][:, 4:] == r[4:]).all()
    # grid order: segments are contiguous, most pixels first, ties in the caller's order; channel fastest inside a segment
    order = [int(seg[0])] + [int(b) for a, b in zip(seg[:-1], seg[1:]) if a != b]
    assert len(order) == len(Ps) and order == sorted(range(len(Ps)), key=lambda k: (-Ps[k], k))
    first = m[seg == order[0]]
    assert (first[:Nf, 1] == np.arange(Nf)).all()


@pytest.mark.parametrize('Nt,Nf,P', [(2, 3, 128), (2, 3, 16448), (8, 256, 98304), (8, 256, 10048), (2, 1536, 32832)])
def test_one_segment_is_the_single_launch_plan(Nt, Nf, P):
    fwd, bwd = block_map(False, Nt, Nf, (P,)), block_map(True, Nt, Nf, (P,))
    assert fwd[:, 3].max() + 1 == kt.fwd_splits(Nt, Nf, P)
    assert bwd[:, 3].max() + 1 == pair_bwd_splits(Nt, Nf, P)[0]
    from bayeslim_amd import ops
    assert bwd[:, 3].max() + 1 == ops.lib.rime_fringe_pair_bwd_splits(Nt, Nf, P)


def test_c4_step():
    """2048 rows; 3072 + 314 panels: six forward splits + one, and in the backward the point sources widen to ONE split on
    the combined grid (alone: two, 4096 blocks; the diffuse launch keeps its three)"""
    fwd, bwd = block_map(False, 8, 256, (98304, 10048)), block_map(True, 8, 256, (98304, 10048))
    assert len(fwd) == 2048 * 7 and (fwd[:2048 * 6, 0] == 0).all() and (fwd[2048 * 6:, 0] == 1).all()
    assert len(bwd) == 2048 * 4 and (bwd[:2048 * 3, 0] == 0).all() and (bwd[2048 * 3:, 0] == 1).all()
    assert (bwd[2048 * 3:, 4] == 0).all() and (bwd[2048 * 3:, 5] == 314).all()
    from bayeslim_amd import ops
    assert ops.lib.rime_fringe_pair_bwd_splits(8, 256, 10048) == 2
    Ps = (ctypes.c_int * 2)(98304, 10048)
    assert ops.lib.rime_fringe_pair_segments_workspace(8128, 8, 256, Ps, 2) == 7 * 8128 * 2048 * 8


def test_refused_shapes():
    from bayeslim_amd import ops
    f = ops.lib.rime_fringe_pair_segments_map
    for Ps in [(), (64,) * 5, (96,), (0,)]:
        arr = (ctypes.c_int * max(len(Ps), 1))(*Ps)
        assert f(0, 2, 3, arr, len(Ps), None, 0) == -1
