"""
Which matrix-core fringe kernel instantiation serves which call (bayeslim_amd/csrc/fringe_mfma.hip), as one table.

KERNELS maps every row -- (instantiation, runtime branch) -- to the C ABI entry point that launches it, an example of the
arguments that select it (checked against `dispatch` by tests/test_fringe_kernel_table.py), the minimum blocks per CU of its
__launch_bounds__, and the case (CASES below) that reaches it.  The branch is '' for a plain row; a
runtime branch inside one instantiation that changes the arithmetic is a row of its own: `accumulate` of the backward kernels
(the block adds to the psky gradient another block wrote) and `mirror` of fringe_ant_bwd_kernel on a real plane (ops never
passes a mirror mask with a complex psky: its blocks are the plain ones).

CASES are the cases of tests/test_fringe_kernels_gpu.py (build_case: their arrays and baselines); LaunchRecorder stands in
for ops.lib and records the block launches.

`dispatch` restates the C dispatch of rime_fringe_ant_{fwd,bwd}_block and rime_fringe_pair_{fwd,bwd}_block: the rows one
accepted call launches, with the default switches of the library (RIME_FWD_PACKED, RIME_BWD_SMALL on).  `grid` restates
the launch grid of the same calls (fwd_split_plan and bwd_split_plan of csrc/fringe_mfma_common.h).

Plain data and host arithmetic only: the CPU tests import it as well as the GPU tests.
"""
import ctypes
import re
import zlib

import numpy as np

FWD, BWD = 'rime_fringe_ant_fwd_block', 'rime_fringe_ant_bwd_block'
PFWD, PBWD = 'rime_fringe_pair_fwd_block', 'rime_fringe_pair_bwd_block'

MF_SPLIT_PIX, MF_KP = 16384, 32           # fringe_mfma_common.h: pixels per forward block at most, pixels per panel

# Argument names of the selecting arguments (include/rime_hip.h): Nrows, cross, mirror, psky_complex, accumulate, and
# rowmin (a non-null row-minimum pointer: real planes) for the forward; centre (a hub slot table) and flat for the pair form.


def _r(entry, args, min_blocks, case):
    return dict(entry=entry, args=args, min_blocks=min_blocks, case=case)


def _fwd(nrows, mirror=0, cross=0, cplx=0):
    return dict(Nrows=nrows, cross=cross, mirror=mirror, psky_complex=cplx, rowmin=not cplx)


def _bwd(nrows, mirror=0, cross=0, cplx=0, acc=0):
    return dict(Nrows=nrows, cross=cross, mirror=mirror, psky_complex=cplx, accumulate=acc)


def _pfwd(nrows, centre, flat):
    return dict(Nrows=nrows, centre=centre, flat=flat, rowmin=True)


def _pbwd(nrows, centre, flat, acc):
    return dict(Nrows=nrows, centre=centre, flat=flat, accumulate=acc)


KERNELS = {
    # diagonal blocks, one real plane per call: TA = ceil(Nrows / 32) row tiles (33..48 rows: the packed kernel), both SIGNED
    # variants (rows with a negative value / rows without), MIR = a mirror mask licenced
    ('fringe_ant_fwd_kernel<1, true, false>', ''): _r(FWD, _fwd(24), 2, 'rand24'),
    ('fringe_ant_fwd_kernel<1, false, false>', ''): _r(FWD, _fwd(24), 2, 'rand24'),
    ('fringe_ant_fwd_kernel<1, true, true>', ''): _r(FWD, _fwd(19, mirror=1), 2, 'hex19'),
    ('fringe_ant_fwd_kernel<1, false, true>', ''): _r(FWD, _fwd(19, mirror=1), 2, 'hex19'),
    ('fringe_ant_fwd_kernel<2, true, false>', ''): _r(FWD, _fwd(60), 2, 'rand60'),
    ('fringe_ant_fwd_kernel<2, false, false>', ''): _r(FWD, _fwd(60), 2, 'rand60'),
    ('fringe_ant_fwd_kernel<2, true, true>', ''): _r(FWD, _fwd(61, mirror=15), 2, 'hex61-mirror'),
    ('fringe_ant_fwd_kernel<2, false, true>', ''): _r(FWD, _fwd(61, mirror=15), 2, 'hex61-mirror'),
    ('fringe_ant_fwd_kernel<3, true, false>', ''): _r(FWD, _fwd(90), 2, 'rand90'),
    ('fringe_ant_fwd_kernel<3, false, false>', ''): _r(FWD, _fwd(90), 2, 'rand90'),
    ('fringe_ant_fwd_kernel<3, true, true>', ''): _r(FWD, _fwd(91, mirror=63), 2, 'hex91-mirror'),
    ('fringe_ant_fwd_kernel<3, false, true>', ''): _r(FWD, _fwd(91, mirror=63), 2, 'hex91-mirror'),
    ('fringe_ant_fwd_kernel<4, true, false>', ''): _r(FWD, _fwd(128), 2, 'rand128'),
    ('fringe_ant_fwd_kernel<4, false, false>', ''): _r(FWD, _fwd(128), 2, 'rand128'),
    ('fringe_ant_fwd_kernel<4, true, true>', ''): _r(FWD, _fwd(128, mirror=127), 2, 'sym128'),
    ('fringe_ant_fwd_kernel<4, false, true>', ''): _r(FWD, _fwd(128, mirror=127), 2, 'sym128'),
    ('fringe_ant_fwd_packed_kernel<true, false>', ''): _r(FWD, _fwd(40), 2, 'rand40'),
    ('fringe_ant_fwd_packed_kernel<false, false>', ''): _r(FWD, _fwd(40), 2, 'rand40'),
    ('fringe_ant_fwd_packed_kernel<true, true>', ''): _r(FWD, _fwd(37, mirror=3), 2, 'hex37-mirror'),
    ('fringe_ant_fwd_packed_kernel<false, true>', ''): _r(FWD, _fwd(37, mirror=3), 2, 'hex37-mirror'),
    # cross blocks (rows_i = cross, rows_j = Nrows - cross): a real plane runs <SIGNED = true, false>, a complex single pass
    # <false, CPLX = true>; 4 x 4 tiles take 8 waves and one block per CU
    ('fringe_ant_fwd_cross_kernel<1, 1, true, false>', ''): _r(FWD, _fwd(64, cross=32), 2, 'beam-models'),
    ('fringe_ant_fwd_cross_kernel<1, 1, false, false>', ''): _r(FWD, _fwd(64, cross=32), 2, 'beam-models'),
    ('fringe_ant_fwd_cross_kernel<1, 1, false, true>', ''): _r(FWD, _fwd(64, cross=32, cplx=1), 2, 'cplx-g32'),
    ('fringe_ant_fwd_cross_kernel<1, 2, true, false>', ''): _r(FWD, _fwd(96, cross=32), 2, 'g64'),
    ('fringe_ant_fwd_cross_kernel<1, 2, false, false>', ''): _r(FWD, _fwd(96, cross=32), 2, 'g64'),
    ('fringe_ant_fwd_cross_kernel<1, 2, false, true>', ''): _r(FWD, _fwd(96, cross=32, cplx=-1), 2, 'g64'),
    ('fringe_ant_fwd_cross_kernel<2, 2, true, false>', ''): _r(FWD, _fwd(128, cross=64), 2, 'g64'),
    ('fringe_ant_fwd_cross_kernel<2, 2, false, false>', ''): _r(FWD, _fwd(128, cross=64), 2, 'g64'),
    ('fringe_ant_fwd_cross_kernel<2, 2, false, true>', ''): _r(FWD, _fwd(128, cross=64, cplx=1), 2, 'g64'),
    ('fringe_ant_fwd_cross_kernel<4, 4, true, false>', ''): _r(FWD, _fwd(256, cross=128), 1, 'rand150'),
    ('fringe_ant_fwd_cross_kernel<4, 4, false, false>', ''): _r(FWD, _fwd(256, cross=128), 1, 'rand150'),
    ('fringe_ant_fwd_cross_kernel<4, 4, false, true>', ''): _r(FWD, _fwd(256, cross=128, cplx=1), 1, 'cplx-g128-up'),
    # self blocks (cross == Nrows): a diagonal block of one pair orientation in ONE complex pass, Nrows = 32 TI
    ('fringe_ant_fwd_self_kernel<1>', ''): _r(FWD, _fwd(32, cross=32, cplx=1), 2, 'cplx-g32'),
    ('fringe_ant_fwd_self_kernel<2>', ''): _r(FWD, _fwd(64, cross=64, cplx=1), 2, 'g64'),
    ('fringe_ant_fwd_self_kernel<3>', ''): _r(FWD, _fwd(96, cross=96, cplx=1), 2, 'cplx-g128-up'),
    ('fringe_ant_fwd_self_kernel<4>', ''): _r(FWD, _fwd(128, cross=128, cplx=1), 1, 'cplx-g128-up'),
    # conjugate-pair form, forward: <= 32 rows without a hub -> the one-tile kernel, else <SIGNED, CEN = hub, FLAT>
    ('fringe_pair_fwd1_kernel<true, true>', ''): _r(PFWD, _pfwd(19, False, True), 2, 'hex37'),
    ('fringe_pair_fwd1_kernel<false, true>', ''): _r(PFWD, _pfwd(19, False, True), 2, 'hex37'),
    ('fringe_pair_fwd1_kernel<true, false>', ''): _r(PFWD, _pfwd(25, False, False), 2, 'sym45'),
    ('fringe_pair_fwd1_kernel<false, false>', ''): _r(PFWD, _pfwd(25, False, False), 2, 'sym45'),
    ('fringe_pair_fwd_kernel<true, false, true>', ''): _r(PFWD, _pfwd(46, False, True), 3, 'hex91+hex127+1+hex91'),
    ('fringe_pair_fwd_kernel<false, false, true>', ''): _r(PFWD, _pfwd(46, False, True), 3, 'hex91+hex127+1+hex91'),
    ('fringe_pair_fwd_kernel<true, false, false>', ''): _r(PFWD, _pfwd(55, False, False), 3, 'sym100+hex127+1t+sym100'),
    ('fringe_pair_fwd_kernel<false, false, false>', ''): _r(PFWD, _pfwd(55, False, False), 3, 'sym100+hex127+1t+sym100'),
    ('fringe_pair_fwd_kernel<true, true, true>', ''): _r(PFWD, _pfwd(64, True, True), 3, 'hex127+1+hex37'),
    ('fringe_pair_fwd_kernel<false, true, true>', ''): _r(PFWD, _pfwd(64, True, True), 3, 'hex127+1+hex37'),
    ('fringe_pair_fwd_kernel<true, true, false>', ''): _r(PFWD, _pfwd(64, True, False), 3, 'hex127+1t+sym45'),
    ('fringe_pair_fwd_kernel<false, true, false>', ''): _r(PFWD, _pfwd(64, True, False), 3, 'hex127+1t+sym45'),
    # backward, diagonal blocks: <CPLX = complex single pass, TAMAX = 2 up to 64 rows, else 4>
    ('fringe_ant_bwd_kernel<false, 2>', 'accumulate=0'): _r(BWD, _bwd(24), 2, 'rand24'),
    ('fringe_ant_bwd_kernel<false, 2>', 'accumulate=1'): _r(BWD, _bwd(22, acc=1), 2, 'rand150'),
    ('fringe_ant_bwd_kernel<false, 2>', 'mirror=0'): _r(BWD, _bwd(24), 2, 'rand24'),
    ('fringe_ant_bwd_kernel<false, 2>', 'mirror=1'): _r(BWD, _bwd(19, mirror=1), 2, 'hex19'),
    ('fringe_ant_bwd_kernel<false, 4>', 'accumulate=0'): _r(BWD, _bwd(128), 2, 'rand128'),
    ('fringe_ant_bwd_kernel<false, 4>', 'accumulate=1'): _r(BWD, _bwd(72, acc=1), 2, 'cplx-g128-down'),
    ('fringe_ant_bwd_kernel<false, 4>', 'mirror=0'): _r(BWD, _bwd(128), 2, 'rand128'),
    ('fringe_ant_bwd_kernel<false, 4>', 'mirror=1'): _r(BWD, _bwd(128, mirror=127), 2, 'sym128'),
    ('fringe_ant_bwd_kernel<true, 2>', 'accumulate=0'): _r(BWD, _bwd(32, cplx=1), 2, 'cplx-g32'),
    ('fringe_ant_bwd_kernel<true, 2>', 'accumulate=1'): _r(BWD, _bwd(32, cplx=1, acc=1), 2, 'cplx-g32'),
    ('fringe_ant_bwd_kernel<true, 4>', 'accumulate=0'): _r(BWD, _bwd(128, cplx=1), 2, 'cplx-g128-up'),
    ('fringe_ant_bwd_kernel<true, 4>', 'accumulate=1'): _r(BWD, _bwd(72, cplx=1, acc=1), 2, 'cplx-g128-up'),
    # backward, cross blocks: accumulate = 0 where the cross block is the first writer of its psky plane (a plane of its
    # own: a beam-model pair that only crosses groups; or the single-pass cross blocks ahead of two-pass diagonal blocks)
    ('fringe_ant_bwd_cross_kernel<false>', 'accumulate=0'): _r(BWD, _bwd(64, cross=32), 2, 'beam-models'),
    ('fringe_ant_bwd_cross_kernel<false>', 'accumulate=1'): _r(BWD, _bwd(256, cross=128, acc=1), 2, 'rand150'),
    ('fringe_ant_bwd_cross_kernel<true>', 'accumulate=0'): _r(BWD, _bwd(256, cross=128, cplx=-1), 2, 'cplx-g128-down'),
    ('fringe_ant_bwd_cross_kernel<true>', 'accumulate=1'): _r(BWD, _bwd(256, cross=128, cplx=1, acc=1), 2, 'cplx-g128-up'),
    # conjugate-pair form, backward: <CEN = hub, FLAT, TF = 1 for <= 32 rows without a hub, else 2>; accumulate = 1 for a
    # pair block behind another block of its psky plane (a second group of antennas)
    ('fringe_pair_bwd_kernel<false, true, 1>', 'accumulate=0'): _r(PBWD, _pbwd(19, False, True, 0), 3, 'hex37'),
    ('fringe_pair_bwd_kernel<false, true, 1>', 'accumulate=1'): _r(PBWD, _pbwd(19, False, True, 1), 3, 'hex127+1+hex37'),
    ('fringe_pair_bwd_kernel<false, false, 1>', 'accumulate=0'): _r(PBWD, _pbwd(25, False, False, 0), 3, 'sym45'),
    ('fringe_pair_bwd_kernel<false, false, 1>', 'accumulate=1'): _r(PBWD, _pbwd(25, False, False, 1), 3, 'hex127+1t+sym45'),
    ('fringe_pair_bwd_kernel<false, true, 2>', 'accumulate=0'): _r(PBWD, _pbwd(46, False, True, 0), 3, 'hex91+hex127+1+hex91'),
    ('fringe_pair_bwd_kernel<false, true, 2>', 'accumulate=1'): _r(PBWD, _pbwd(46, False, True, 1), 3, 'hex91+hex127+1+hex91'),
    ('fringe_pair_bwd_kernel<false, false, 2>', 'accumulate=0'): _r(PBWD, _pbwd(55, False, False, 0), 3, 'sym100+hex127+1t+sym100'),
    ('fringe_pair_bwd_kernel<false, false, 2>', 'accumulate=1'): _r(PBWD, _pbwd(55, False, False, 1), 3, 'sym100+hex127+1t+sym100'),
    ('fringe_pair_bwd_kernel<true, true, 2>', 'accumulate=0'): _r(PBWD, _pbwd(64, True, True, 0), 3, 'hex127+1+hex37'),
    ('fringe_pair_bwd_kernel<true, true, 2>', 'accumulate=1'): _r(PBWD, _pbwd(64, True, True, 1), 3, 'hex91+hex127+1+hex91'),
    ('fringe_pair_bwd_kernel<true, false, 2>', 'accumulate=0'): _r(PBWD, _pbwd(64, True, False, 0), 3, 'hex127+1t+sym45'),
    ('fringe_pair_bwd_kernel<true, false, 2>', 'accumulate=1'): _r(PBWD, _pbwd(64, True, False, 1), 3, 'sym100+hex127+1t+sym100'),
}

# the other kernels of fringe_mfma.hip and the entry points that launch them
SIDE_KERNELS = {
    'row_scale_kernel': 'rime_fringe_row_scale',
    'row_scale_cplx_kernel': 'rime_fringe_row_scale_cplx',
    'reduce_vis_kernel': 'rime_fringe_ant_fwd_finish',
    'transpose_gvis_kernel': 'rime_fringe_ant_bwd_prepare',
}


def instantiations():
    """the instantiation names of the table (one per kernel, whatever its runtime rows)"""
    return {k for k, _ in KERNELS}


def short_name(demangled):
    """'void rime::fringe_ant_fwd_kernel<1, true, false>(rime::AntArgs)' -> 'fringe_ant_fwd_kernel<1, true, false>'"""
    s = re.sub(r'^void\s+', '', demangled.strip())
    s = re.sub(r'^rime::', '', s)
    depth = 0
    for i, ch in enumerate(s):              # cut the parameter list (the first '(' outside the template arguments)
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            return s[:i]
    return s


def _b(x):
    return 'true' if x else 'false'


def dispatch(entry, a):
    """rows (instantiation, branch) that one accepted call of `entry` launches; `a` holds the selecting arguments by their
    C names (see KERNELS), pointers as truth values"""
    n = int(a['Nrows'])
    if entry == FWD:
        cross, cplx = int(a['cross']), int(a['psky_complex'])
        if cross and cross == n:
            return [('fringe_ant_fwd_self_kernel<%d>' % (n // 32), '')]
        if cross:
            ti, tj = cross // 32, (n - cross) // 32
            if (ti, tj) not in ((1, 1), (1, 2), (2, 2)):
                ti = tj = 4
            k = 'fringe_ant_fwd_cross_kernel<%d, %d, %%s, %%s>' % (ti, tj)
            if cplx:
                return [(k % ('false', 'true'), '')]
            return [(k % ('true', 'false'), '')] + ([(k % ('false', 'false'), '')] if a['rowmin'] else [])
        assert not cplx, 'a diagonal block takes one real plane per call'
        mirror = int(a['mirror'])
        ta = min((n + 31) // 32, 4)
        if ta == 2 and n <= 48:
            mirror &= 3
            k = 'fringe_ant_fwd_packed_kernel<%s, ' + _b(mirror) + '>'
        else:
            k = 'fringe_ant_fwd_kernel<%d, %%s, %s>' % (ta, _b(mirror))
        return [(k % 'true', '')] + ([(k % 'false', '')] if a['rowmin'] else [])
    if entry == BWD:
        acc = 'accumulate=%d' % int(bool(a['accumulate']))
        cplx = _b(a['psky_complex'])
        if a['cross']:
            return [('fringe_ant_bwd_cross_kernel<%s>' % cplx, acc)]
        k = 'fringe_ant_bwd_kernel<%s, %d>' % (cplx, 2 if n <= 64 else 4)
        rows = [(k, acc)]
        if not a['psky_complex']:
            rows.append((k, 'mirror=%d' % int(a['mirror'] != 0)))
        return rows
    if entry == PFWD:
        flat = _b(a['flat'])
        if n <= 32 and not a['centre']:
            k = 'fringe_pair_fwd1_kernel<%s, ' + flat + '>'
        else:
            k = 'fringe_pair_fwd_kernel<%s, ' + _b(a['centre']) + ', ' + flat + '>'
        return [(k % 'true', '')] + ([(k % 'false', '')] if a['rowmin'] else [])
    if entry == PBWD:
        tf = 1 if (n <= 32 and not a['centre']) else 2
        return [('fringe_pair_bwd_kernel<%s, %s, %d>' % (_b(a['centre']), _b(a['flat']), tf),
                 'accumulate=%d' % int(bool(a['accumulate'])))]
    raise KeyError(entry)


def fwd_splits(Nt, Nf, Pstride):
    """S of the forward launches (fwd_split_plan): grid = Nt S Nf"""
    S = (Pstride + MF_SPLIT_PIX - 1) // MF_SPLIT_PIX
    maxS = max(1, Pstride // 1024)
    while Nt * Nf * S < 1024 and S < maxS:
        S += 1
    S = max(1, S)
    npanel = Pstride // MF_KP
    pps = (npanel + S - 1) // S
    pps = ((pps + 3) // 4) * 4
    return (npanel + pps - 1) // pps


def fwd_split_pixels(Nt, Nf, Pstride):
    """pixels per forward split (the last split holds the rest)"""
    S = fwd_splits(Nt, Nf, Pstride)
    npanel = Pstride // MF_KP
    return ((((npanel + S - 1) // S) + 3) // 4) * 4 * MF_KP


def bwd_splits(Nt, Nf, Pstride):
    """(S, pixels per split) of the backward launches (bwd_split_plan)"""
    ntile = Pstride // 32
    per = 256
    while per > 8 and Nt * Nf * ((ntile + per - 1) // per) < 1024:
        per //= 2
    return (ntile + per - 1) // per, 32 * per


def grid(entry, Nt, Nf, Pstride):
    """blocks of one launch of `entry`"""
    S = fwd_splits(Nt, Nf, Pstride) if entry in (FWD, PFWD) else bwd_splits(Nt, Nf, Pstride)[0]
    return Nt * S * Nf


# ---- launch recorder ---------------------------------------------------------------------------------------------------
# argument positions (include/rime_hip.h) of the selecting arguments, the pair_direct table and the (Nt, Nf, Pstride) shape
_ARGS = {
    FWD: dict(Nrows=1, cross=2, mirror=3, rowmin=8, direct=9, Nt=12, Nf=13, Pstride=14, psky_complex=19),
    BWD: dict(Nrows=1, cross=2, mirror=3, direct=7, Nt=10, Nf=11, Pstride=12, psky_complex=17, accumulate=18),
    PFWD: dict(Nrows=1, centre=2, flat=3, rowmin=8, direct=9, Nt=12, Nf=13, Pstride=14),
    PBWD: dict(Nrows=1, centre=2, flat=3, direct=7, Nt=10, Nf=11, Pstride=12, accumulate=17),
}


def _value(x):
    return x.value if isinstance(x, ctypes.c_void_p) else x


class LaunchRecorder:
    """stands in for ops.lib: forwards every call to the real ctypes function and records the accepted block launches as
    (entry, selecting arguments)"""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _ARGS:
            return fn

        def call(*args):
            rc = fn(*args)
            if rc == 0:
                self.calls.append((name, {k: _value(args[i]) for k, i in _ARGS[name].items()}))
            return rc
        return call

    def rows(self):
        """(row, entry, arguments) of every recorded launch"""
        return [(row, entry, a) for entry, a in self.calls for row in dispatch(entry, a)]


# ---- arrays ------------------------------------------------------------------------------------------------------------
HEX_SIDE = {'hex19': 3, 'hex37': 4, 'hex61': 5, 'hex91': 6, 'hex127': 7}
SYM = {'sym45': (20, 5), 'sym100': (45, 10), 'sym128': (60, 8)}       # mirror pairs, antennas without a partner (tilted)


def _positions(kind, rng):
    """antenna positions of one group: 'randN' random, 'hexN' a coplanar hexagon (+1: an outrigger, so that the centre
    antenna becomes the hub of the conjugate-pair form; t: tilted out of its plane), 'symN' random mirror pairs + singles;
    the point-symmetric ones about a centre away from the origin"""
    from bayeslim_amd import utils
    if kind.startswith('rand'):
        return rng.normal(0, 80.0, (int(kind[4:]), 3)) * [1, 1, 0.02]
    if kind.startswith('hex'):
        base = kind.split('+')[0].rstrip('t')
        ant = np.asarray(utils._make_hex(HEX_SIDE[base], D=14.6)[1])
        if '+1' in kind:
            ant = np.vstack([ant, [[250.0, 3.0, 0.0]]])
        if kind.endswith('t'):
            a = np.deg2rad(3.0)
            ant = ant @ np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]).T
    else:
        half, single = SYM[kind]
        h = rng.normal(0, 70.0, (half, 3)) * [1, 1, 0.05]
        ant = np.vstack([h, -h, rng.normal(0, 70.0, (single, 3)) * [1, 1, 0.05]])
    return ant[rng.permutation(len(ant))] + np.array([31.7, -12.3, 4.1])


# case id -> groups of antennas (each but the last padded to 128 with antennas that hold no baseline, so that the next one
# starts a group of its own; baselines only inside a group) or one array cut into groups of `group`, psky kind(s), P
CASES = {
    'rand24': dict(arrays=['rand24'], P=17000),
    'rand40': dict(arrays=['rand40'], P=17000, conj=True),
    'rand60': dict(arrays=['rand60']),
    'rand90': dict(arrays=['rand90'], conj=True),
    'rand128': dict(arrays=['rand128'], frac=0.7),
    'rand150': dict(arrays=['rand150'], frac=0.5, conj=True),
    'hex19': dict(arrays=['hex19'], P=17000, conj=True),
    'hex37': dict(arrays=['hex37'], P=17000),
    'hex37-mirror': dict(arrays=['hex37'], P=17000, pair=False, conj=True),
    'hex61': dict(arrays=['hex61'], conj=True),
    'hex61-mirror': dict(arrays=['hex61'], pair=False),
    'hex91-mirror': dict(arrays=['hex91'], pair=False, conj=True),
    'hex127': dict(arrays=['hex127'], frac=0.7),
    'sym45': dict(arrays=['sym45'], P=17000, conj=True),
    'sym128': dict(arrays=['sym128'], frac=0.7),
    'hex127+1+hex37': dict(arrays=['hex127+1', 'hex37'], frac=0.6),
    'hex127+1t+sym45': dict(arrays=['hex127+1t', 'sym45'], frac=0.6, conj=True),
    'hex91+hex127+1+hex91': dict(arrays=['hex91', 'hex127+1', 'hex91'], frac=0.4),
    'sym100+hex127+1t+sym100': dict(arrays=['sym100', 'hex127+1t', 'sym100'], frac=0.4, conj=True),
    'beam-models': dict(arrays=['rand60'], models=2, conj=True),
    'cplx-g32': dict(arrays=['rand100'], group=32, frac=0.7, orient='up', psky=('complex',)),
    'g64': dict(arrays=['rand160'], group=64, frac=0.4, orient='up', psky=('real', 'complex')),
    'cplx-g128-up': dict(arrays=['rand200'], frac=0.4, orient='up', psky=('complex',), conj=True),
    'cplx-g128-down': dict(arrays=['rand200'], frac=0.4, orient='down', psky=('complex',)),
}


def build_case(cid):
    """host side of a case: antenna positions, baselines as antenna pairs, beam-model index per baseline and pair table"""
    spec = CASES[cid]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    ants, pairs, offset = [], [], 0
    for k, kind in enumerate(spec['arrays']):
        pos = _positions(kind, rng)
        n = len(pos)
        hub = None
        if '+1' in kind:                              # the antenna at the centre: its autocorrelation declines the pair form
            hub = int(np.argmin(np.abs(pos - pos.mean(0)).sum(1)))
        p = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < spec.get('frac', 0.9)]
        orient = spec.get('orient')
        p = [(i, j) if orient == 'up' else ((j, i) if orient == 'down' or rng.random() < 0.5 else (i, j)) for i, j in p]
        p += [(a, a) for a in range(0, n, 17) if a != hub][:3]            # autocorrelations
        pairs += [(offset + i, offset + j) for i, j in p]
        ants.append(pos)
        if k + 1 < len(spec['arrays']):               # idle antennas fill the group: the next array is a group of its own
            assert n <= 128
            ants.append(rng.normal(0, 80.0, (128 - n, 3)) * [1, 1, 0.02])
            n = 128
        offset += n
    ant = np.vstack(ants)
    pairs = [pairs[k] for k in rng.permutation(len(pairs))]
    bl_mp, mp_pairs = None, None
    if spec.get('models'):
        # beam model a % models: the groups follow the models, so baselines between models form cross blocks of planes
        # no diagonal block writes (accumulate = 0 on the cross kernels)
        model = [a % spec['models'] for a in range(len(ant))]
        mp_pairs = sorted({(model[a], model[b]) for a, b in pairs})
        bl_mp = [mp_pairs.index((model[a], model[b])) for a, b in pairs]
    return ant, pairs, bl_mp, mp_pairs
