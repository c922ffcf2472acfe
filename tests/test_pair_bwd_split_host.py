"""Pixel splits of the conjugate-pair backward (pair_bwd_split_plan of csrc/fringe_mfma_common.h, through
rime_fringe_pair_bwd_splits): wider splits on large grids only, the generic backward plan everywhere else.  CPU only."""
import pytest

import fringe_kernel_table as kt

MIN_GRID = 8 * 3 * 256           # PAIR_BWD_MIN_GRID: 8 rounds of 3 blocks on each of 256 CUs


def pair_bwd_splits(Nt, Nf, Pstride):
    """pair_bwd_split_plan restated: (S, tiles per split)"""
    ntile = Pstride // 32
    per = kt.bwd_splits(Nt, Nf, Pstride)[1] // 32
    while 256 <= per < 1024 and Nt * Nf * ((ntile + 2 * per - 1) // (2 * per)) >= MIN_GRID:
        per *= 2
    return (ntile + per - 1) // per, per


# (Nt, Nf, Pstride, splits): the C4 diffuse launch (12 splits of 256 tiles before) and its point-source launch (10 000
# sources padded to 10 048: too few blocks to widen); the thresholds of the rule on both sides; the shapes of
# test_fringe_kernel_table.test_split_plans
TABLE = [
    (8, 256, 98304, 3), (8, 256, 10048, 2),
    (8, 256, 49152, 3),            # 1536 tiles: 512 per split (1024 would leave 4096 blocks)
    (8, 128, 98304, 6),            # 1024 rows: 512 per split, 6144 blocks
    (8, 128, 98240, 6),            # ragged last split
    (8, 96, 98304, 12),            # 768 rows: 6 splits would leave 4608 blocks -- unchanged
    (16, 256, 98304, 3), (64, 256, 32768, 1),
    (3, 520, 1024, 1), (3, 520, 17024, 3), (2, 7, 17024, 67), (1, 1, 98304, 384),
]


@pytest.mark.parametrize('Nt,Nf,P,S', TABLE)
def test_pair_bwd_splits(Nt, Nf, P, S):
    from bayeslim_amd import ops
    got = ops.lib.rime_fringe_pair_bwd_splits(Nt, Nf, P)
    assert got == S == pair_bwd_splits(Nt, Nf, P)[0]
    base, px = kt.bwd_splits(Nt, Nf, P)
    # never more blocks than the generic plan; the same plan wherever that one has fewer than 2 x MIN_GRID blocks or
    # splits narrower than 256 tiles (tests/fringe_kernel_table.grid, which restates the generic plan, is exact there)
    assert got <= base
    if Nt * Nf * base < 2 * MIN_GRID or px < 256 * 32:
        assert got == base
    else:
        assert Nt * Nf * got >= MIN_GRID
    # every tile belongs to exactly one split
    per = pair_bwd_splits(Nt, Nf, P)[1]
    assert (got - 1) * per < P // 32 <= got * per


def test_pair_bwd_splits_refuses_what_the_block_entry_refuses():
    from bayeslim_amd import ops
    f = ops.lib.rime_fringe_pair_bwd_splits
    assert f(0, 4, 1024) == 0 and f(4, 0, 1024) == 0 and f(4, 4, 0) == 0 and f(-1, 4, 1024) == 0
    assert f(4, 4, 1000) == 0 and f(4, 4, 32) == 0          # Pstride: multiples of 64
    assert f(65536, 4, 1024) == 0 and f(65535, 4, 1024) > 0


def test_switch_selects_the_generic_plan():
    """RIME_PAIR_BWD_WIDE=0 (read once by the library, hence a process of its own): bwd_split_plan, query and launch alike"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('from bayeslim_amd import _lib; f = _lib.lib.rime_fringe_pair_bwd_splits; '
            'print(f(8, 256, 98304), f(8, 256, 10048), f(2, 1536, 32832))')
    for wide, want in (('0', '12 2 5'), ('1', '3 2 2'), ('', '3 2 2')):
        env = dict(os.environ, RIME_PAIR_BWD_WIDE=wide)
        if not wide:
            del env['RIME_PAIR_BWD_WIDE']
        r = subprocess.run([sys.executable, '-c', code], cwd=root, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split('\n')[-2].strip() == want, (wide, r.stdout, r.stderr[-2000:])


def test_signature_is_declared():
    import ctypes
    from bayeslim_amd import _lib
    assert _lib.SIGNATURES['rime_fringe_pair_bwd_splits'] == (ctypes.c_int, [ctypes.c_int] * 3)
