"""
The table of vector-ALU fringe kernel instantiations (tests/fringe_valu_table.py) against the binary this build ships, its
restated dispatch and launch plans against the library's host side, and the cases of tests/test_fringe_valu_gpu.py against
the table -- without a GPU.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import fringe_valu_table as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, 'bayeslim_amd', 'lib', 'obj', 'fringe-hip-amdgcn-amd-amdhsa-gfx950.s')


def _kernels_in_assembly():
    """short demangled names of the .amdhsa_kernel symbols of the gfx950 assembly the build keeps (-save-temps)"""
    if not os.path.exists(ASM):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'bayeslim_amd', 'csrc')], check=True, capture_output=True)
    syms = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', open(ASM).read(), flags=re.M)
    out = subprocess.run(['c++filt'], input='\n'.join(syms), capture_output=True, text=True, check=True).stdout
    names = [vt.short_name(s) for s in out.splitlines() if s.strip()]
    assert len(names) == len(syms) == len(set(names))
    return set(names)


def test_table_names_every_kernel_of_the_binary():
    """every kernel of fringe.hip in the shipped assembly has a row and every row a kernel: 25 + 15 forward and as many
    backward instantiations, four reductions, two gen_fringe kernels"""
    names = _kernels_in_assembly()
    assert names - set(vt.KERNELS) == set(), 'kernels without a table row'
    assert set(vt.KERNELS) - names == set(), 'table rows without a kernel'
    count = lambda head: sum(n.startswith(head) for n in names)
    assert count('fringe_fwd_kernel<float') == 25 and count('fringe_fwd_kernel<double') == 15
    assert count('fringe_bwd_kernel<float') == 25 and count('fringe_bwd_kernel<double') == 15
    assert count('reduce_') == 4 and count('gen_fringe_kernel<') == 2
    assert len(names) == 86


def test_table_rows_follow_the_c_dispatch():
    """the example arguments of every fringe row select that row through `dispatch`; every row names a case, and that
    case states the row among the ones it launches"""
    for row, info in vt.KERNELS.items():
        assert info['case'] in vt.CASES, row
        assert row in vt.expected_rows(info['case']), (row, info['case'])
        if row.startswith('fringe_'):
            a = info['args']
            assert vt.dispatch(a['dtype'], a['Npp'], a['cplx'], a['uniform'], a['max_blen'], a['dfreq'],
                               info['entry'] == vt.SBWD) == row, (row, info)
        else:
            assert row.endswith('<%s>' % vt.CTYPE[info['args']['dtype']])


def test_dispatch_restates_the_c_dispatch_rules():
    """consequences of fringe.hip's dispatch at its switches, spelled out"""
    c = vt.C_LIGHT
    fwd = lambda **kw: vt.dispatch(**dict(dict(dtype='f32', Npp=1, cplx=0, uniform=1, max_blen=100.0, dfreq=1e6,
                                               backward=False), **kw))
    # the 0.3-turn switch from both sides, whatever the direction of the grid
    assert fwd(max_blen=0.299 * c / 1e6) == 'fringe_fwd_kernel<float, 1, false, 32, 2, 0, 1>'
    assert fwd(max_blen=0.301 * c / 1e6) == 'fringe_fwd_kernel<float, 1, false, 32, 1, 0, 1>'
    assert fwd(max_blen=0.299 * c / 1e6, dfreq=-1e6) == 'fringe_fwd_kernel<float, 1, false, 32, 2, 0, 1>'
    assert fwd(max_blen=0.301 * c / 1e6, dfreq=-1e6, uniform=2) == 'fringe_fwd_kernel<float, 1, false, 32, 3, 0, 1>'
    assert fwd(max_blen=0.299 * c / 1e6, uniform=2) == 'fringe_fwd_kernel<float, 1, false, 32, 4, 0, 1>'
    # an unknown longest baseline never takes the shear rotation; one channel (step 0) does
    assert fwd(max_blen=0.0) == 'fringe_fwd_kernel<float, 1, false, 32, 1, 0, 1>'
    assert fwd(max_blen=-1.0, uniform=2) == 'fringe_fwd_kernel<float, 1, false, 32, 3, 0, 1>'
    assert fwd(max_blen=5000.0, dfreq=0.0) == 'fringe_fwd_kernel<float, 1, false, 32, 2, 0, 1>'
    # the grid flag: 0 = arbitrary grid, one sincos per channel, whatever the step
    assert fwd(uniform=0, max_blen=10.0) == 'fringe_fwd_kernel<float, 1, false, 32, 0, 0, 1>'
    # float64 has no shear kernels: LIFT -> ROT, LIFT_NU -> ROT_NU
    assert fwd(dtype='f64', max_blen=10.0) == 'fringe_fwd_kernel<double, 1, false, 16, 1, 0, 1>'
    assert fwd(dtype='f64', max_blen=10.0, uniform=2) == 'fringe_fwd_kernel<double, 1, false, 16, 3, 0, 1>'
    assert fwd(dtype='f64', max_blen=1e4, uniform=2) == 'fringe_fwd_kernel<double, 1, false, 16, 3, 0, 1>'
    # chunk geometry
    assert fwd(Npp=2) == 'fringe_fwd_kernel<float, 2, false, 16, 1, 0, 1>'
    assert fwd(Npp=4, cplx=1, dtype='f64') == 'fringe_fwd_kernel<double, 4, true, 4, 1, 0, 1>'
    with pytest.raises(vt.Unsupported):
        fwd(Npp=2, cplx=1)
    with pytest.raises(vt.Unsupported):
        fwd(Npp=3)
    # backward: WPS = 4 only in float32 where NPP * NC * CH <= 32, and never for MODE_DIRECT
    bwd = lambda **kw: fwd(backward=True, **kw)
    assert bwd() == 'fringe_bwd_kernel<float, 1, false, 32, 1, 1, 4>'
    assert bwd(Npp=4) == 'fringe_bwd_kernel<float, 4, false, 8, 1, 1, 4>'
    assert bwd(Npp=4, cplx=1) == 'fringe_bwd_kernel<float, 4, true, 8, 1, 1, 1>'
    assert bwd(uniform=0) == 'fringe_bwd_kernel<float, 1, false, 32, 0, 1, 1>'
    assert bwd(dtype='f64') == 'fringe_bwd_kernel<double, 1, false, 16, 1, 1, 1>'
    assert {vt.wps('f32', cfg, 'LIFT') for cfg in ('r1', 'r2', 'c1', 'r4')} == {4} and vt.wps('f32', 'c4', 'LIFT') == 1


def test_library_declines_two_complex_planes():
    """Npp = 2 with a complex psky is RIME_EUNSUPPORTED (validated on the host before any launch)"""
    from bayeslim_amd import ops
    one = ctypes.c_void_p(64)                      # non-null pointers nobody follows: the call returns at its validation
    off = (ctypes.c_int * 2)(0, 5)
    for fn in (ops.lib.rime_fringe_sum_fwd, ops.lib.rime_fringe_sum_bwd):
        rc = fn(0, one, one, one, one, off, None, 5, 1, 4, 64, 1, 2, 1, 1, 1, 1.5e8, 1e6, 100.0, None, one, one, 0, None)
        assert rc == -4


SHAPES = [(Nbl, Nt, Nf, Ps) for Nbl in (1, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 700, 5000)
          for Nt in (1, 3, 128) for Nf in (1, 7, 33, 520) for Ps in (64, 128, 192, 256, 320, 704, 1472, 16384, 270336)]


def test_workspace_restates_the_library():
    """the restated workspace equals rime_fringe_sum_workspace over shapes on both sides of every block-size and split
    boundary, for every plane configuration, type and direction"""
    from bayeslim_amd import ops
    seen = set()
    for Nbl, Nt, Nf, Ps in SHAPES:
        for dtype, code in (('f32', 0), ('f64', 1)):
            for cfg, (Npp, cplx) in vt.CONFIGS.items():
                for backward in (0, 1):
                    want = ops.lib.rime_fringe_sum_workspace(code, Nbl, Nt, Nf, Ps, 1, Npp, int(cplx), backward)
                    got = vt.workspace(dtype, Nbl, Nt, Nf, Ps, 1, Npp, cplx, backward)
                    assert got == want, (dtype, cfg, backward, Nbl, Nt, Nf, Ps, got, want)
                    seen.add((backward, got > 0))
    assert seen == {(0, False), (0, True), (1, False), (1, True)}


def test_plans_at_their_boundaries():
    """block sizes, split counts and grids of the restated plans at the values fringe.hip switches on"""
    assert [vt.fwd_block(n) for n in (1, 64, 65, 128, 129, 192, 193, 256, 257, 1000)] == [
        64, 64, 128, 128, 192, 192, 256, 256, 256, 256]
    assert [vt.bwd_block(p) for p in (64, 128, 192, 256, 320)] == [64, 128, 192, 256, 256]
    # forward: at least four tiles per split; the last split may be ragged (11 tiles = 6 + 5; 23 = 4 x 5 + 3)
    assert vt.plan_fwd(70, 2, 33, 192, 32) == dict(S=1, tiles=3, block=128)
    assert vt.plan_fwd(70, 2, 33, 704, 32) == dict(S=2, tiles=6, block=128)
    assert vt.plan_fwd(70, 2, 9, 1472, 4) == dict(S=5, tiles=5, block=128)
    # more than FLUSH_TILES tiles per split
    assert vt.plan_fwd(3, 128, 1, 270336, 32) == dict(S=128, tiles=33, block=64)
    # enough waves: no split
    assert vt.plan_fwd(5000, 128, 520, 16384, 32)['S'] == 1
    assert vt.pick_splits(vt.SPLIT_TARGET - 1, 8) == 2 and vt.pick_splits(vt.SPLIT_TARGET, 8) == 1
    # backward: a group without baselines is one (empty) tile; 64 / 65 baselines: one / two tiles
    assert vt.plan_bwd(0, 2, 40, 256, 32) == dict(S=1, tiles=1, block=256)
    assert vt.plan_bwd(64, 2, 40, 256, 32)['S'] == 1 and vt.plan_bwd(65, 2, 40, 256, 32)['S'] == 2
    assert vt.plan_bwd(257, 1, 9, 256, 32) == dict(S=5, tiles=1, block=256)
    # the split count is rounded to whole tiles per split: 9 tiles in at most 4 splits -> 3 + 3 + 3
    assert vt.plan_bwd(9 * 64, 4096, 1, 64, 32) == dict(S=3, tiles=3, block=64)
    assert vt.grid_fwd(70, 300, 3, 33, 704, 32) == (1 * 3 * vt.plan_fwd(300, 3, 33, 704, 32)['S'], 2, 128)
    assert vt.grid_bwd(130, 3, 20, 192, 16) == (1 * 3 * 3, 2, 192)


@pytest.mark.parametrize('Nbl', [1, 64, 65, 300, 1031, 4097])
def test_group_plans_fit_the_workspace(Nbl):
    """every model-pair group plans its own backward splits; whatever its size g <= Nbl, its partial slabs fit the
    workspace the library sizes from Nbl alone"""
    from bayeslim_amd import ops
    for dtype, code, tsz in (('f32', 0, 4), ('f64', 1, 8)):
        for cfg, (Npp, cplx) in vt.CONFIGS.items():
            CH = vt.CHUNK[dtype][cfg]
            for Nt, Nf, Ps in ((1, 1, 64), (2, 33, 320), (3, 520, 1024), (60, 64, 4096), (7, 2 * CH + 1, 192)):
                bound = ops.lib.rime_fringe_sum_workspace(code, Nbl, Nt, Nf, Ps, 3, Npp, int(cplx), 1)
                plane = Npp * Nf * Ps * (2 if cplx else 1)
                for g in range(Nbl + 1):
                    S = vt.plan_bwd(g, Nt, Nf, Ps, CH)['S']
                    assert S == 1 or S * Nt * plane * tsz <= bound, (dtype, cfg, Nbl, g, Nt, Nf, Ps, S, bound)


def test_gpu_cases_reach_every_table_row_on_the_host(monkeypatch):
    """the cases of tests/test_fringe_valu_gpu.py run through ops' launch sequence with a library stand-in that accepts
    every launch (CPU tensors, nothing computed): each case reaches exactly the rows it states, the rows the table assigns
    to it among them, and together they reach every row.  The GPU module asserts the same on the real launches."""
    from bayeslim_amd import ops
    real = ops.lib

    class HostOnlyLib:
        """the library's host-side workspace sizes as they are; every other call accepted, nothing launched"""
        def __getattr__(self, name):
            fn = getattr(real, name)
            return fn if 'workspace' in name else (lambda *args: 0)

    fake = vt.LaunchRecorder(HostOnlyLib())
    monkeypatch.setattr(ops, 'lib', fake)
    monkeypatch.setattr(ops, '_require_cuda', lambda *a: None)
    monkeypatch.setattr(ops, '_stream', lambda: ctypes.c_void_p(0))
    reached = set()
    for cid, spec in vt.CASES.items():
        c = vt.build_case(cid, sky=False)
        Ps = ops.pad_to_tile(spec['P'])
        f64 = spec['dtype'] == 'f64'
        rdt, cdt = (torch.float64, torch.complex128) if f64 else (torch.float32, torch.complex64)
        fake.calls.clear()
        if spec.get('gen'):
            ops.gen_fringe(torch.as_tensor(c['blvecs']), torch.zeros(3, spec['P'], dtype=torch.float64), c['freqs'],
                           dtype=rdt)
        else:
            geom = ops.FringeGeometry(torch.as_tensor(c['blvecs']), torch.zeros(spec['Nt'], 3, Ps, dtype=torch.float64),
                                      c['freqs'], bl_mp=c['bl_mp'], Nmp=c['Nmp'], conj=spec['conj'])
            x = torch.zeros((spec['Nt'], c['Nmp'], c['Npp'], spec['Nf'], Ps), dtype=cdt if c['cplx'] else rdt)
            v = torch.zeros((c['Npp'], c['Nbl'], spec['Nt'], spec['Nf']), dtype=cdt)
            if not spec.get('adjoint'):
                ops._fringe_call_planes(geom, False, x, v, c['cplx'])
            ops._fringe_call_planes(geom, True, x, v, c['cplx'])
        rows = {row for row, _, _ in fake.rows()}
        assert rows == vt.expected_rows(cid), (cid, sorted(rows ^ vt.expected_rows(cid)))
        mine = {row for row, info in vt.KERNELS.items() if info['case'] == cid}
        assert mine <= rows, (cid, sorted(mine - rows))
        reached |= rows
    assert reached == set(vt.KERNELS), sorted(set(vt.KERNELS) ^ reached)
