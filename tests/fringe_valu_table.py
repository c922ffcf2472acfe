"""
Which vector-ALU fringe kernel instantiation serves which call (bayeslim_amd/csrc/fringe.hip), as one table.

KERNELS maps every kernel of fringe.hip in the binary -- fringe_fwd_kernel<T, NPP, CPLX, CH, MODE, 0, 1>,
fringe_bwd_kernel<T, NPP, CPLX, CH, MODE, 1, WPS>, reduce_partials_kernel<T>, reduce_bwd_kernel<T>, gen_fringe_kernel<T> --
to the C ABI entry point that launches it, an example of the arguments that select it (checked against `dispatch` by
tests/test_fringe_valu_table.py) and the case (CASES below) that reaches it.

`dispatch` restates the choice fringe.hip makes inside the library: the chunk geometry (ChunkOf), the rotation mode
(fringe_common: LIFT below 0.3 turn per channel, float64 folds the shear modes onto the rotation modes) and WPS.
`plan_fwd` / `plan_bwd` / `workspace` restate the launch plans and rime_fringe_sum_workspace.

CASES are the cases of tests/test_fringe_valu_gpu.py (build_case: their arrays); LaunchRecorder stands in for ops.lib and
maps the recorded calls through `dispatch` and the plans to table rows.

Plain data and host arithmetic only: the CPU tests import it as well as the GPU tests.
"""
import zlib

import numpy as np

C_LIGHT = 2.99792458e8
SFWD, SBWD, GEN = 'rime_fringe_sum_fwd', 'rime_fringe_sum_bwd', 'rime_gen_fringe'

TP = TB = 64                      # fringe.hip: pixels per forward LDS tile, baselines per backward LDS tile
FLUSH_TILES = 32                  # accumulators go to memory every 32 tiles
SPLIT_TARGET = 16384              # pick_splits: waves the split plans aim at
LIFT_STEP = 0.3                   # fringe_common: the shear rotation below this many turns per channel

MODES = {'DIRECT': 0, 'ROT': 1, 'LIFT': 2, 'ROT_NU': 3, 'LIFT_NU': 4}
CTYPE = {'f32': 'float', 'f64': 'double'}
# (Npp, complex psky) -> short name, channels per lane (ChunkOf<float>, ChunkOf<double>)
CONFIGS = {'r1': (1, False), 'r2': (2, False), 'c1': (1, True), 'r4': (4, False), 'c4': (4, True)}
CHUNK = {'f32': {'r1': 32, 'r2': 16, 'c1': 16, 'r4': 8, 'c4': 8},
         'f64': {'r1': 16, 'r2': 8, 'c1': 8, 'r4': 4, 'c4': 4}}
# the modes each type instantiates (launch_fwd_t / launch_bwd_t: float64 has no shear kernels)
TYPE_MODES = {'f32': ('DIRECT', 'ROT', 'LIFT', 'ROT_NU', 'LIFT_NU'), 'f64': ('DIRECT', 'ROT', 'ROT_NU')}


class Unsupported(Exception):
    """the library answers RIME_EUNSUPPORTED"""


def _b(x):
    return 'true' if x else 'false'


def config_of(Npp, cplx):
    for k, v in CONFIGS.items():
        if v == (int(Npp), bool(cplx)):
            return k
    raise Unsupported('Npp = %d, complex = %s' % (Npp, bool(cplx)))      # Npp = 2 complex (fringe_common)


def wps(dtype, cfg, mode):
    """waves per SIMD of the backward's __launch_bounds__: 4 for the float32 kernels of at most 32 accumulators, but the
    MODE_DIRECT ones"""
    Npp, cplx = CONFIGS[cfg]
    return 4 if (dtype == 'f32' and Npp * (2 if cplx else 1) * CHUNK[dtype][cfg] <= 32 and mode != 'DIRECT') else 1


def kernel_name(dtype, cfg, mode, backward):
    Npp, cplx = CONFIGS[cfg]
    head = 'fringe_%s_kernel<%s, %d, %s, %d, %d' % ('bwd' if backward else 'fwd', CTYPE[dtype], Npp, _b(cplx),
                                                     CHUNK[dtype][cfg], MODES[mode])
    return head + (', 1, %d>' % wps(dtype, cfg, mode) if backward else ', 0, 1>')


def select_mode(dtype, uniform, max_blen, dfreq):
    """the mode fringe_common picks from the grid flag (0 arbitrary, 1 uniform, 2 near uniform), the longest baseline
    (<= 0: unknown) and the channel step, with float64's folding of the shear modes"""
    if uniform not in (1, 2):
        return 'DIRECT'
    nu = uniform == 2
    mode = 'ROT_NU' if nu else 'ROT'
    if max_blen > 0 and max_blen * abs(dfreq / C_LIGHT) < LIFT_STEP:
        mode = 'LIFT_NU' if nu else 'LIFT'
    if dtype == 'f64':
        mode = {'LIFT': 'ROT', 'LIFT_NU': 'ROT_NU'}.get(mode, mode)
    return mode


def dispatch(dtype, Npp, cplx, uniform, max_blen, dfreq, backward):
    """the fringe kernel one accepted rime_fringe_sum_{fwd,bwd} call launches"""
    cfg = config_of(Npp, cplx)
    return kernel_name(dtype, cfg, select_mode(dtype, uniform, max_blen, dfreq), backward)


# ---- launch plans ------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def pick_splits(waves, max_splits):
    if waves >= SPLIT_TARGET or max_splits <= 1:
        return 1
    return max(1, min(_cdiv(SPLIT_TARGET, waves), max_splits))


def fwd_block(bl_cnt):
    return 256 if bl_cnt >= 256 else _cdiv(bl_cnt, 64) * 64


def plan_fwd(Nbl, Nt, Nf, Pstride, CH):
    """one pixel-split plan per call, from the whole baseline count: dict(S, tiles, block)"""
    block = fwd_block(Nbl)
    waves = _cdiv(Nbl, block) * (block // 64) * _cdiv(Nf, CH) * Nt
    ntiles = Pstride // TP
    S = pick_splits(waves, max(1, ntiles // 4))
    tiles = _cdiv(ntiles, S)
    return dict(S=_cdiv(ntiles, tiles), tiles=tiles, block=block)


def bwd_block(Pstride):
    return 256 if Pstride >= 256 else _cdiv(Pstride, 64) * 64


def plan_bwd(bl_cnt, Nt, Nf, Pstride, CH):
    """the baseline-split plan of one model-pair group (PIX = 1); a group without baselines still launches"""
    block = bwd_block(Pstride)
    waves = _cdiv(Pstride, block) * (block // 64) * _cdiv(Nf, CH) * Nt
    ntiles = max(1, _cdiv(bl_cnt, TB))
    S = pick_splits(waves, ntiles)
    tiles = _cdiv(ntiles, S)
    return dict(S=_cdiv(ntiles, tiles), tiles=tiles, block=block)


def grid_fwd(bl_cnt, Nbl, Nt, Nf, Pstride, CH):
    """(blocks in x, blocks in y, threads) of one group's forward launch"""
    pl = plan_fwd(Nbl, Nt, Nf, Pstride, CH)
    block = fwd_block(bl_cnt)
    return _cdiv(bl_cnt, block) * Nt * pl['S'], _cdiv(Nf, CH), block


def grid_bwd(bl_cnt, Nt, Nf, Pstride, CH):
    pl = plan_bwd(bl_cnt, Nt, Nf, Pstride, CH)
    return _cdiv(Pstride, pl['block']) * Nt * pl['S'], _cdiv(Nf, CH), pl['block']


def workspace(dtype, Nbl, Nt, Nf, Pstride, Nmp, Npp, cplx, backward):
    """bytes rime_fringe_sum_workspace asks for: S slabs of the visibilities (forward), or of one model pair's gradient
    plane with the un-rounded split count of the largest possible group (backward)"""
    tsz = 8 if dtype == 'f64' else 4
    CH = CHUNK[dtype][config_of(Npp, cplx)]
    if not backward:
        S = plan_fwd(Nbl, Nt, Nf, Pstride, CH)['S']
        return 0 if S <= 1 else S * Npp * Nbl * Nt * Nf * 2 * tsz
    block = bwd_block(Pstride)
    waves = _cdiv(Pstride, block) * (block // 64) * _cdiv(Nf, CH) * Nt
    S = pick_splits(waves, _cdiv(Nbl, TB))
    return 0 if S <= 1 else S * Nt * Npp * Nf * Pstride * (2 if cplx else 1) * tsz


# ---- the table ---------------------------------------------------------------------------------------------------------
def _args(dtype, cfg, uniform, max_blen, dfreq):
    Npp, cplx = CONFIGS[cfg]
    return dict(dtype=dtype, Npp=Npp, cplx=int(cplx), uniform=uniform, max_blen=max_blen, dfreq=dfreq)


# example grids per mode: flag, longest baseline [m], channel step [Hz] (1 MHz: 0.3 turn at 89.9 m)
_EXAMPLE = {'DIRECT': (0, 200.0, 0.0), 'ROT': (1, 200.0, 1e6), 'LIFT': (1, 60.0, 1e6), 'ROT_NU': (2, 200.0, 1e6),
            'LIFT_NU': (2, 60.0, 1e6)}


def _build_table():
    tab = {}
    for dtype in ('f32', 'f64'):
        for cfg in CONFIGS:
            for mode in TYPE_MODES[dtype]:
                case = '%s-%s-%s' % (dtype, cfg, mode.lower())
                for backward in (False, True):
                    tab[kernel_name(dtype, cfg, mode, backward)] = dict(
                        entry=SBWD if backward else SFWD, args=_args(dtype, cfg, *_EXAMPLE[mode]), case=case)
    # the reductions behind a split plan, and the materialised fringe
    tab['reduce_partials_kernel<float>'] = dict(entry=SFWD, args=dict(dtype='f32', split=True), case='fwd-split-ragged')
    tab['reduce_partials_kernel<double>'] = dict(entry=SFWD, args=dict(dtype='f64', split=True), case='fwd-split-ragged-f64-c4')
    tab['reduce_bwd_kernel<float>'] = dict(entry=SBWD, args=dict(dtype='f32', split=True), case='strided-split-bwd-f32-c1')
    tab['reduce_bwd_kernel<double>'] = dict(entry=SBWD, args=dict(dtype='f64', split=True), case='strided-split-bwd-f64-r2')
    tab['gen_fringe_kernel<float>'] = dict(entry=GEN, args=dict(dtype='f32'), case='gen-fringe-f32')
    tab['gen_fringe_kernel<double>'] = dict(entry=GEN, args=dict(dtype='f64'), case='gen-fringe-f64')
    return tab


KERNELS = _build_table()


def short_name(demangled):
    """'void rime::reduce_bwd_kernel<float>(float const*, ...)' -> 'reduce_bwd_kernel<float>'"""
    from fringe_kernel_table import short_name as _short
    return _short(demangled)


# ---- launch recorder ---------------------------------------------------------------------------------------------------
# argument positions (include/rime_hip.h)
_ARGS = {
    SFWD: dict(dtype=0, mp_off=5, bl_order=6, Nbl=7, Nt=8, Nf=9, Pstride=10, Nmp=11, Npp=12, cplx=13, sign=14, uniform=15,
               freq0=16, dfreq=17, max_blen=18, strides=19, ws_bytes=22),
    GEN: dict(dtype=0, Nbl=4, Nf=5, P=6),
}
_ARGS[SBWD] = _ARGS[SFWD]


def _value(x):
    return x.value if hasattr(x, 'value') else x


def launched_rows(entry, a):
    """the table rows one accepted call launches: `a` holds the arguments by their C names, dtype as 'f32' / 'f64',
    mp_off as a list"""
    if entry == GEN:
        return ['gen_fringe_kernel<%s>' % CTYPE[a['dtype']]]
    dtype, backward = a['dtype'], entry == SBWD
    k = dispatch(dtype, a['Npp'], a['cplx'], a['uniform'], a['max_blen'], a['dfreq'], backward)
    CH = CHUNK[dtype][config_of(a['Npp'], a['cplx'])]
    counts = [a['mp_off'][g + 1] - a['mp_off'][g] for g in range(a['Nmp'])]
    rows = []
    if backward:
        rows.append(k)
        if any(plan_bwd(c, a['Nt'], a['Nf'], a['Pstride'], CH)['S'] > 1 for c in counts):
            rows.append('reduce_bwd_kernel<%s>' % CTYPE[dtype])
    else:
        if any(c > 0 for c in counts):
            rows.append(k)
        if plan_fwd(a['Nbl'], a['Nt'], a['Nf'], a['Pstride'], CH)['S'] > 1:
            rows.append('reduce_partials_kernel<%s>' % CTYPE[dtype])
    return rows


class LaunchRecorder:
    """stands in for ops.lib: forwards every call to the real ctypes function and records the accepted calls of
    rime_fringe_sum_fwd / _bwd / rime_gen_fringe as (entry, arguments)"""

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
                a = {k: _value(args[i]) for k, i in _ARGS[name].items()}
                a['dtype'] = 'f64' if a['dtype'] == 1 else 'f32'
                if 'mp_off' in a:
                    a['mp_off'] = [int(a['mp_off'][g]) for g in range(a['Nmp'] + 1)]
                    a['strides'] = None if a['strides'] is None else [int(s) for s in a['strides']]
                    a['bl_order'] = bool(a['bl_order'])
                self.calls.append((name, a))
            return rc
        return call

    def rows(self):
        """(row, entry, arguments) of every recorded launch"""
        return [(row, entry, a) for entry, a in self.calls for row in launched_rows(entry, a)]


# ---- cases -------------------------------------------------------------------------------------------------------------
# A case: dtype, cfg (CONFIGS), the MODE its kernels are instantiated with (stated, not derived), the channel grid
#   grid = 'uniform' | 'near' (uniform + residuals of size `phi` = 2 pi eps max_blen / c) | 'ragged' (sorted random)
#   step = max_blen |df| / c in turns (fixes the longest baseline for the given df [Hz]; df < 0: descending grid), or blen [m]
# Nf, Nt, P (valid pixels; the axis is padded to 64), groups = baselines per model pair (0: a pair without baselines),
# conj, strided (time-inner storage passed as a permuted view), adjoint (ops.fringe_adjoint only), gen (ops.gen_fringe only),
# repeat (runs that must agree bit for bit), splits = the reductions the plans launch ('fwd', 'bwd'), stated.
def _case(dtype, cfg, mode, grid='uniform', step=None, df=1e6, blen=None, phi=None, Nf=None, Nt=2, P=300, groups=(90,),
          conj=False, splits=None, **kw):
    if Nf is None:
        Nf = 2 * CHUNK[dtype][cfg] + 1            # two full chunks (whole rotation chains) and a last chunk of one channel
    if splits is None:                           # small pixel axes: one forward split; a group of 65..128 baselines: two tiles
        splits = ('bwd',) if max(groups) > 64 else ()
    return dict(dtype=dtype, cfg=cfg, mode=mode, grid=grid, step=step, df=df, blen=blen, phi=phi, Nf=Nf, Nt=Nt, P=P,
                groups=tuple(groups), conj=conj, splits=tuple(splits), **kw)


def _build_cases():
    cs = {}
    # every (T, NPP, CPLX) x MODE: LIFT modes at 0.29 turn (the largest step they are given), float32 ROT modes on km
    # baselines (26 turns), near-uniform float32 grids at phi = 1.9e-3 (the acceptance bound of FringeGeometry is 2e-3),
    # float64 ones at 5e-7 (beyond 1e-6 a float64 call takes the MODE_DIRECT kernels, ops.NU_F64_PHI)
    for i, cfg in enumerate(CONFIGS):
        groups = (50, 40) if CONFIGS[cfg][1] else (90,)
        kw = dict(groups=groups, conj=bool(i % 2))
        cs['f32-%s-direct' % cfg] = _case('f32', cfg, 'DIRECT', 'ragged', blen=300.0, **kw)
        cs['f32-%s-rot' % cfg] = _case('f32', cfg, 'ROT', step=26.0, **kw)
        cs['f32-%s-lift' % cfg] = _case('f32', cfg, 'LIFT', step=0.29, **kw)
        cs['f32-%s-rot_nu' % cfg] = _case('f32', cfg, 'ROT_NU', 'near', step=26.0, phi=1.9e-3, **kw)
        cs['f32-%s-lift_nu' % cfg] = _case('f32', cfg, 'LIFT_NU', 'near', step=0.29, df=1e4, phi=1.9e-3, **kw)
        cs['f32-%s-rot-0.31' % cfg] = _case('f32', cfg, 'ROT', step=0.31, **kw)
        kw['conj'] = not kw['conj']
        cs['f64-%s-direct' % cfg] = _case('f64', cfg, 'DIRECT', 'ragged', blen=300.0, **kw)
        cs['f64-%s-rot' % cfg] = _case('f64', cfg, 'ROT', step=2.0, **kw)
        cs['f64-%s-rot_nu' % cfg] = _case('f64', cfg, 'ROT_NU', 'near', step=2.0, phi=5e-7, **kw)
    # near-uniform grids at small phi (a float32-rounded linspace on 200 m: phi ~ 3e-5)
    cs['f32-r1-lift_nu-smallphi'] = _case('f32', 'r1', 'LIFT_NU', 'near', step=0.2, df=3e5, phi=3e-5)
    cs['f32-c1-rot_nu-smallphi'] = _case('f32', 'c1', 'ROT_NU', 'near', step=0.6, df=1e6, phi=3e-5, groups=(50, 40))
    # float64 beyond its near-uniform contract: the MODE_DIRECT kernels
    cs['f64-r1-near-phi3e-5'] = _case('f64', 'r1', 'DIRECT', 'near', step=0.6, phi=3e-5)
    cs['f64-r1-near-phi1.9e-3'] = _case('f64', 'r1', 'DIRECT', 'near', step=26.0, phi=1.9e-3, km=True, conj=True, Nf=64)
    cs['f64-c4-near-phi1.9e-3'] = _case('f64', 'c4', 'DIRECT', 'near', step=26.0, phi=1.9e-3, km=True, groups=(50, 40))
    # float64 below 0.3 turn: the rotation kernels all the same; km baselines in float64
    cs['f64-r1-step0.29'] = _case('f64', 'r1', 'ROT', step=0.29)
    cs['f64-r1-rot-km'] = _case('f64', 'r1', 'ROT', step=26.0, km=True, conj=True)
    cs['f32-c4-direct-km'] = _case('f32', 'c4', 'DIRECT', 'ragged', blen=7800.0, groups=(50, 40))
    # Npp = 2 complex: the library declines it, ops runs the planes one by one
    cs['f32-c2-planes'] = _case('f32', 'c1', 'LIFT', step=0.25, Npp=2, groups=(40,))
    # the last chunk: Nf = 1, CH - 1, CH, CH + 1 for every CH (anchor channel beyond Nf, one full chunk, a chunk of one)
    for dtype, cfg, mode in (('f32', 'r1', 'LIFT'), ('f32', 'r2', 'LIFT'), ('f32', 'r4', 'LIFT'), ('f64', 'r1', 'ROT'),
                             ('f64', 'r4', 'ROT')):
        CH = CHUNK[dtype][cfg]
        for Nf in (1, CH - 1, CH, CH + 1):
            kw = dict(blen=100.0) if Nf == 1 else dict(step=0.29 if mode == 'LIFT' else 1.3)
            cs['%s-%s-nf%d' % (dtype, cfg, Nf)] = _case(dtype, cfg, mode, Nf=Nf, groups=(50,), P=200, **kw)
    # descending grids
    cs['desc-f32-r1-lift'] = _case('f32', 'r1', 'LIFT', step=0.29, df=-1e4)
    cs['desc-f32-c1-rot'] = _case('f32', 'c1', 'ROT', step=2.0, df=-1e6, groups=(50, 40), conj=True)
    cs['desc-f32-r2-lift_nu'] = _case('f32', 'r2', 'LIFT_NU', 'near', step=0.25, df=-1e5, phi=1e-3)
    cs['desc-f64-r1-rot'] = _case('f64', 'r1', 'ROT', step=2.0, df=-1e6)
    cs['desc-f64-c1-rot_nu'] = _case('f64', 'c1', 'ROT_NU', 'near', step=2.0, df=-1e6, phi=5e-7, groups=(50, 40))
    # block sizes 64 / 128 / 192 / 256 of the forward and 1..5 baseline tiles of the backward: group sizes around 64 and 256
    sizes = (1, 63, 64, 65, 129, 192, 193, 255, 256, 257)
    cs['group-sizes-f32'] = _case('f32', 'r1', 'LIFT', step=0.29, Nt=1, Nf=9, P=200, groups=sizes, splits=('bwd',))
    cs['group-sizes-f64'] = _case('f64', 'r2', 'ROT', step=2.0, Nt=1, Nf=9, P=200, groups=sizes, splits=('bwd',), conj=True)
    # the pixel axis: one tile (Pstride = 64) and the backward's block sizes
    for P in (50, 100, 190, 300):
        cs['pstride-%d' % (_cdiv(P, 64) * 64)] = _case('f32', 'r1', 'LIFT', step=0.29, Nf=33, P=P, groups=(50,))
    cs['pstride-64-f64-c1'] = _case('f64', 'c1', 'ROT', step=2.0, Nf=9, P=64, groups=(30, 20))
    # a model pair without baselines, in first, middle and last position (with split and unsplit neighbours)
    cs['empty-first'] = _case('f32', 'r1', 'LIFT', step=0.29, Nf=40, P=200, groups=(0, 70, 60))
    cs['empty-middle'] = _case('f32', 'c1', 'ROT', step=2.0, Nf=40, P=200, groups=(70, 0, 60))
    cs['empty-last'] = _case('f32', 'r4', 'LIFT_NU', 'near', step=0.25, df=1e5, phi=1e-3, Nf=20, P=200, groups=(70, 60, 0))
    cs['empty-middle-f64-c4'] = _case('f64', 'c4', 'ROT', step=2.0, Nf=9, P=200, groups=(70, 0, 0, 60))
    # time-inner storage read and written in place, several model pairs, baseline-split backward; three identical runs
    cs['strided-split-bwd-f32-c1'] = _case('f32', 'c1', 'ROT', step=2.0, Nt=3, Nf=20, P=150, groups=(130, 65, 105),
                                           strided=True, repeat=3)
    cs['strided-split-bwd-f64-r2'] = _case('f64', 'r2', 'ROT', step=2.0, Nt=3, Nf=20, P=150, groups=(130, 65, 105),
                                           strided=True, conj=True)
    cs['strided-f32-r4-lift'] = _case('f32', 'r4', 'LIFT', step=0.29, Nt=3, Nf=20, P=150, groups=(40, 60), strided=True)
    # forward pixel splits with a ragged last split: 11 tiles = 6 + 5; 23 tiles = 4 x 5 + 3; three identical runs
    cs['fwd-split-ragged'] = _case('f32', 'r1', 'LIFT', step=0.29, Nf=33, P=700, groups=(70,), splits=('fwd', 'bwd'),
                                   repeat=3)
    cs['fwd-split-ragged-f64-c4'] = _case('f64', 'c4', 'ROT', step=2.0, Nf=9, P=1470, groups=(40, 30), splits=('fwd',),
                                          conj=True)
    cs['fwd-split-ragged-f32-c1-nu'] = _case('f32', 'c1', 'ROT_NU', 'near', step=1.0, phi=1e-3, Nf=20, P=1470,
                                             groups=(40, 30), splits=('fwd',))
    # more than 2048 pixels per split: 4224 tiles in 128 splits of 33 tiles -- one flush inside the loop, one after it
    cs['fwd-flush'] = _case('f32', 'r1', 'LIFT', blen=100.0, Nt=128, Nf=1, P=270300, groups=(3,), splits=('fwd',))
    # map making (no autograd) and the materialised fringe
    cs['adjoint-f32-r2'] = _case('f32', 'r2', 'LIFT', step=0.29, groups=(90,), adjoint=True)
    cs['adjoint-f64-r1'] = _case('f64', 'r1', 'ROT', step=2.0, groups=(90,), adjoint=True, conj=True)
    cs['gen-fringe-f32'] = _case('f32', 'r1', 'DIRECT', 'ragged', blen=300.0, Nt=1, Nf=19, gen=True, groups=(40,), splits=())
    cs['gen-fringe-f64'] = _case('f64', 'r1', 'DIRECT', 'ragged', blen=300.0, Nt=1, Nf=19, gen=True, groups=(40,), splits=(),
                                 conj=True)
    return cs


CASES = _build_cases()


def expected_rows(cid):
    """the table rows the case launches, from what the case states"""
    spec = CASES[cid]
    T = CTYPE[spec['dtype']]
    if spec.get('gen'):
        return {'gen_fringe_kernel<%s>' % T}
    rows = {kernel_name(spec['dtype'], spec['cfg'], spec['mode'], True)}
    if 'bwd' in spec['splits']:
        rows.add('reduce_bwd_kernel<%s>' % T)
    if not spec.get('adjoint'):
        rows.add(kernel_name(spec['dtype'], spec['cfg'], spec['mode'], False))
        if 'fwd' in spec['splits']:
            rows.add('reduce_partials_kernel<%s>' % T)
    return rows


def build_case(cid, sky=True):
    """host side of a case (numpy, float64): blvecs (Nbl, 3), freqs (Nf,), bl_mp (Nbl,), and with sky=True zenaz (Nt, 2, P)
    [deg], psky (Nt, Nmp, Npp, Nf, P) (values exact in the case's dtype) and gvis (Npp, Nbl, Nt, Nf)"""
    spec = CASES[cid]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    Nbl, Nmp, Nf, Nt, P = sum(spec['groups']), len(spec['groups']), spec['Nf'], spec['Nt'], spec['P']
    Npp, cplx = CONFIGS[spec['cfg']]
    Npp = spec.get('Npp', Npp)
    # channel grid
    df = float(spec['df'])
    if spec['grid'] == 'ragged':
        freqs = np.sort(rng.uniform(100e6, 200e6, Nf))
        if df < 0:
            freqs = freqs[::-1].copy()
    else:
        freqs = 150e6 + df * np.arange(Nf)
    # baselines: the longest one has the length the step asks for
    blen = spec['blen'] if spec['blen'] is not None else spec['step'] * C_LIGHT / abs(df)
    blvecs = rng.normal(0, 1.0, (Nbl, 3)) * [1, 1, 0.05]
    blvecs *= blen / np.linalg.norm(blvecs, axis=1).max()
    if spec['grid'] == 'near':
        eps = spec['phi'] * C_LIGHT / (2 * np.pi * blen)
        u = rng.uniform(-1, 1, Nf)
        u[0] = u[-1] = 0.0                        # the end channels define the fitted grid
        u[1 + int(rng.integers(Nf - 2))] = 1.0   # the largest residual is eps itself
        freqs = freqs + eps * u
    bl_mp = rng.permutation(np.repeat(np.arange(Nmp), spec['groups']))       # bl_order: not the identity
    out = dict(blvecs=blvecs, freqs=freqs, bl_mp=bl_mp, Nbl=Nbl, Nmp=Nmp, Npp=Npp, cplx=cplx, blen=blen)
    if not sky:
        return out
    f32 = spec['dtype'] == 'f32'

    def values(shape):
        x = rng.normal(size=shape)
        return x.astype(np.float32).astype(np.float64) if f32 else x

    out['zenaz'] = np.stack([np.rad2deg(np.arccos(rng.uniform(0.0, 1.0, (Nt, P)))), rng.uniform(0, 360, (Nt, P))], axis=1)
    shape = (Nt, Nmp, Npp, Nf, P)
    env = np.exp(-6.0 * rng.uniform(size=shape))                            # beam-like: a few decades of envelope
    psky = values(shape) * env
    if cplx:
        psky = psky + 1j * values(shape) * env
    if f32:
        psky = psky.astype(np.complex64 if cplx else np.float32).astype(np.complex128 if cplx else np.float64)
    out['psky'] = psky
    out['gvis'] = values((Npp, Nbl, Nt, Nf)) + 1j * values((Npp, Nbl, Nt, Nf))
    return out
