"""
The return code of every REJECTED call of the matrix-core fringe block entry points (include/rime_hip.h), as one table --
without a GPU.

Each row is a call that the validation of its entry point turns away before anything is launched: the arguments of an
acceptable call (BASE) with one or two of them made bad.  Rows with two faults pin the ORDER of the checks: null pointers,
then shapes and flags (RIME_EINVAL), the complex pass on a diagonal block (RIME_EUNSUPPORTED), and the workspace
(RIME_EWORKSPACE) -- which the backward of the generic blocks checks BEFORE the mirror mask and the forward after it.
The acceptable call itself is never made: the pointers are those of a small host buffer.
"""
import ctypes

import pytest

from bayeslim_amd import _lib

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4

FWD, BWD = 'rime_fringe_ant_fwd_block', 'rime_fringe_ant_bwd_block'
PFWD, PBWD = 'rime_fringe_pair_fwd_block', 'rime_fringe_pair_bwd_block'
XFWD, XBWD = 'rime_fringe_pair_cross_fwd_block', 'rime_fringe_pair_cross_bwd_block'
FINISH = 'rime_fringe_ant_fwd_finish'

_BUF = ctypes.create_string_buffer(4096)
PTR = ctypes.addressof(_BUF)

# one (t, f) row of 64 pixels, five baselines: the forward workspace is one slab of 5 x 2 floats, the backward's the same
SHAPE = dict(Nbl=5, Nt=1, Nf=1, Pstride=64, st_t=64, st_f=64, st_p=1, sign=1)
WS_BYTES = 40
_FWD_IN = dict(sdir=PTR, freqs=PTR, psky=PTR, scale=PTR, rowmin=PTR, pair_direct=PTR, pair_conj=PTR)
_BWD_IN = dict(sdir=PTR, freqs=PTR, gscale=PTR, pair_direct=PTR, pair_conj=PTR)
_WS = dict(workspace=PTR, workspace_bytes=WS_BYTES, stream=None)

# arguments in the order of the C declarations
BASE = {
    FWD: dict(antpos=PTR, Nrows=40, cross=0, mirror=0, **_FWD_IN, **SHAPE, psky_complex=0, **_WS),
    BWD: dict(antpos=PTR, Nrows=40, cross=0, mirror=0, **_BWD_IN, **SHAPE, psky_complex=0, accumulate=0, gpsky=PTR, **_WS),
    PFWD: dict(antpos=PTR, Nrows=40, centre=None, flat=0, **_FWD_IN, **SHAPE, **_WS),
    PBWD: dict(antpos=PTR, Nrows=40, centre=None, flat=0, **_BWD_IN, **SHAPE, accumulate=0, gpsky=PTR, **_WS),
    XFWD: dict(antpos=PTR, rows_i=40, rows_j=24, flat=0, **_FWD_IN, **SHAPE, **_WS),
    XBWD: dict(antpos=PTR, rows_i=40, rows_j=24, flat=0, **_BWD_IN, **SHAPE, accumulate=0, gpsky=PTR, **_WS),
    FINISH: dict(workspace=PTR, workspace_bytes=WS_BYTES, vis=PTR, Nbl=5, Nt=1, Nf=1, Pstride=64, stream=None),
}
ALL_BLOCKS = (FWD, BWD, PFWD, PBWD, XFWD, XBWD)
# pointers an entry point requires (rowmin and centre may be null: a row without a minimum, a block without a hub)
REQUIRED = {e: [k for k, v in BASE[e].items() if v == PTR and k not in ('rowmin', 'workspace')] for e in ALL_BLOCKS}

NO_WS = dict(workspace=None)
SHORT_WS = dict(workspace_bytes=WS_BYTES - 1)


def _rows():
    rows = []

    def add(entry, code, **bad):
        rows.append((entry, bad, code))

    for e in ALL_BLOCKS:
        for name in REQUIRED[e]:                                     # null pointers, one at a time
            add(e, EINVAL, **{name: None})
        add(e, EINVAL, antpos=None, **NO_WS)                         # ... ahead of the workspace
        add(e, EINVAL, pair_conj=None, st_p=3)
        for bad in (dict(st_p=3), dict(st_p=0), dict(Pstride=63), dict(Pstride=0), dict(Nt=65536), dict(Nt=0),
                    dict(Nf=0), dict(Nbl=0), dict(sign=0), dict(sign=2)):
            add(e, EINVAL, **bad)
            add(e, EINVAL, **bad, **NO_WS)                           # shapes and flags ahead of the workspace
        add(e, EWORKSPACE, **NO_WS)
        add(e, EWORKSPACE, **SHORT_WS)
        add(e, EWORKSPACE, workspace_bytes=0)
    # row counts: a generic block holds 1..128 rows, a pair block 1..64, a pair cross block 1..64 a side
    for e in (FWD, BWD):
        for n in (0, -1, 129):
            add(e, EINVAL, Nrows=n)
        add(e, EINVAL, Nrows=129, **SHORT_WS)
    for e in (PFWD, PBWD):
        for n in (0, 65, 129):
            add(e, EINVAL, Nrows=n)
        add(e, EINVAL, Nrows=65, **SHORT_WS)
    for e in (XFWD, XBWD):
        for n in (0, 65, 129):
            add(e, EINVAL, rows_i=n)
            add(e, EINVAL, rows_j=n)
        add(e, EINVAL, rows_i=65, rows_j=0)
        add(e, EINVAL, rows_j=65, **NO_WS)
    # generic blocks: cross shapes other than 32 x 32, 32 x 64, 64 x 64, 128 x 128; self blocks (cross == Nrows) need a complex
    # psky and 32 / 64 / 96 / 128 rows; a complex psky is interleaved (st_p 2) and flagged +-1
    for e in (FWD, BWD):
        for cross, n in ((64, 96), (32, 48), (16, 48), (128, 192), (96, 192), (32, 160)):
            add(e, EINVAL, cross=cross, Nrows=n)
        add(e, EINVAL, cross=64, Nrows=96, **NO_WS)
        add(e, EINVAL, cross=64, Nrows=64)                           # self block on a real plane
        add(e, EINVAL, cross=48, Nrows=48, psky_complex=1, st_p=2)
        add(e, EINVAL, cross=160, Nrows=160, psky_complex=1, st_p=2)
        add(e, EINVAL, psky_complex=1)                               # st_p 1
        add(e, EINVAL, psky_complex=-1, cross=32, Nrows=64)
        add(e, EINVAL, psky_complex=2, st_p=2)
        add(e, EINVAL, psky_complex=2, st_p=2, cross=32, Nrows=64, **SHORT_WS)
    # the complex pass on a diagonal block: the forward takes one real plane per call, and says so before it looks at the mirror
    # mask or the workspace; the backward has that pass
    add(FWD, EUNSUPPORTED, psky_complex=1, st_p=2)
    add(FWD, EUNSUPPORTED, psky_complex=-1, st_p=2, mirror=-1)
    add(FWD, EUNSUPPORTED, psky_complex=1, st_p=2, mirror=8)
    add(FWD, EUNSUPPORTED, psky_complex=1, st_p=2, **NO_WS)
    add(FWD, EINVAL, psky_complex=1, st_p=2, Nrows=129)
    add(BWD, EWORKSPACE, psky_complex=1, st_p=2, **SHORT_WS)
    # mirror mask: a bit at or beyond ceil(Nrows / 16), or a negative mask; the forward checks it before the workspace, the
    # backward after it
    for e in (FWD, BWD):
        add(e, EINVAL, mirror=8)                                     # 40 rows: bits 0..2
        add(e, EINVAL, mirror=-1)
        add(e, EINVAL, Nrows=128, mirror=256)
        add(e, EINVAL, Nrows=16, mirror=2)
        add(e, EINVAL, cross=32, Nrows=64, mirror=16)                # checked on cross blocks too, where it is not used
    add(FWD, EINVAL, mirror=8, **NO_WS)
    add(FWD, EINVAL, mirror=-1, **SHORT_WS)
    add(BWD, EWORKSPACE, mirror=8, **NO_WS)
    add(BWD, EWORKSPACE, mirror=-1, **SHORT_WS)
    # the reduction of the forward slabs
    for bad in (dict(vis=None), dict(Nbl=0), dict(Nt=0), dict(Nf=0), dict(Pstride=0), dict(Pstride=63), dict(Pstride=96)):
        add(FINISH, EINVAL, **bad)
        add(FINISH, EINVAL, **bad, **NO_WS)
    add(FINISH, EWORKSPACE, **NO_WS)
    add(FINISH, EWORKSPACE, **SHORT_WS)
    return rows


ROWS = _rows()


def _id(row):
    entry, bad, _ = row
    return entry[len('rime_fringe_'):] + '-' + '-'.join('%s=%s' % kv for kv in bad.items())


def test_table_holds_rejections_only():
    """no row expects a code that a call can return after a launch, every row changes an argument of its entry point, and
    all six block entry points and the reduction are in the table"""
    assert {e for e, _, _ in ROWS} == set(BASE)
    for entry, bad, code in ROWS:
        assert code in (EINVAL, EWORKSPACE, EUNSUPPORTED)
        assert bad and set(bad) <= set(BASE[entry]), (entry, bad)
        assert len(BASE[entry]) == len(_lib.SIGNATURES[entry][1])
    assert len({_id(r) for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize('row', ROWS, ids=_id)
def test_rejected_call_returns_its_code(row):
    entry, bad, code = row
    args = dict(BASE[entry], **bad)
    assert getattr(_lib.lib, entry)(*args.values()) == code


@pytest.mark.parametrize('Nt,Nf,P,S', [(3, 520, 1024, 1), (3, 520, 17024, 2), (2, 7, 17024, 15), (1, 1, 98304, 96),
                                       (1, 1, 64, 1), (3, 520, 64, 1), (70, 600, 64 * 7000, 28)])
def test_workspace_queries(Nt, Nf, P, S):
    """bytes of the forward slabs, S pixel splits x (Nt, Nf, re | im, Nbl) floats, and of the backward's transposed gradient"""
    for Nbl in (1, 5, 666):
        assert _lib.lib.rime_fringe_ant_workspace(Nbl, Nt, Nf, P) == S * Nbl * Nt * Nf * 8
        assert _lib.lib.rime_fringe_ant_bwd_workspace(Nbl, Nt, Nf) == Nbl * Nt * Nf * 8
