"""
The table of matrix-core fringe kernel instantiations (tests/fringe_kernel_table.py) against the binary this build ships,
and the cases of tests/test_fringe_kernels_gpu.py against the table -- without a GPU.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import fringe_kernel_table as kt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, 'bayeslim_amd', 'lib', 'obj', 'fringe_mfma-hip-amdgcn-amd-amdhsa-gfx950.s')


def _kernels_in_assembly():
    """short demangled names of the .amdhsa_kernel symbols of the gfx950 assembly the build keeps (-save-temps)"""
    if not os.path.exists(ASM):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'bayeslim_amd', 'csrc')], check=True, capture_output=True)
    syms = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', open(ASM).read(), flags=re.M)
    out = subprocess.run(['c++filt'], input='\n'.join(syms), capture_output=True, text=True, check=True).stdout
    names = [kt.short_name(s) for s in out.splitlines() if s.strip()]
    assert len(names) == len(syms) == len(set(names))
    return set(names)


def test_table_names_every_fringe_kernel_of_the_binary():
    """every fringe_* kernel of the shipped assembly has a row and every row a kernel; the other kernels are the side
    kernels the table lists with their entry points"""
    names = _kernels_in_assembly()
    fringe = {n for n in names if n.startswith('fringe_')}
    assert fringe - kt.instantiations() == set(), 'kernels without a table row'
    assert kt.instantiations() - fringe == set(), 'table rows without a kernel'
    assert names - fringe == set(kt.SIDE_KERNELS)
    assert len(fringe) == 60


def test_table_rows_follow_the_c_dispatch():
    """the example arguments of every row select that row through `dispatch` (the restated C dispatch), each entry point
    is the one that launches the row's kind, and every runtime branch of an instantiation is a row"""
    for row, info in kt.KERNELS.items():
        assert row in kt.dispatch(info['entry'], info['args']), (row, info)
        assert info['min_blocks'] in (1, 2, 3)
        assert info['case'] in kt.CASES, row
    # the backward kernels: both values of `accumulate`; fringe_ant_bwd_kernel on a real plane: both of `mirror`
    for name in kt.instantiations():
        branches = {b for k, b in kt.KERNELS if k == name}
        if '_bwd_' in name:
            want = {'accumulate=0', 'accumulate=1'}
            if name.startswith('fringe_ant_bwd_kernel<false'):
                want |= {'mirror=0', 'mirror=1'}
            assert branches == want, (name, branches)
        else:
            assert branches == {''}, (name, branches)


def test_dispatch_restates_the_c_dispatch_rules():
    """a few consequences of fringe_mfma.hip's dispatch, spelled out"""
    real = dict(cross=0, mirror=0, psky_complex=0, rowmin=True)
    # a real plane launches both SIGNED variants, one without a row minimum only the signed one
    assert len(kt.dispatch(kt.FWD, dict(real, Nrows=70))) == 2
    assert kt.dispatch(kt.FWD, dict(real, Nrows=70, rowmin=False)) == [('fringe_ant_fwd_kernel<3, true, false>', '')]
    # 33..48 rows: the packed kernel, its mirror licence cut to the first row tile
    assert kt.dispatch(kt.FWD, dict(real, Nrows=48, mirror=4))[0] == ('fringe_ant_fwd_packed_kernel<true, false>', '')
    assert kt.dispatch(kt.FWD, dict(real, Nrows=49, mirror=4))[0] == ('fringe_ant_fwd_kernel<2, true, true>', '')
    # a complex cross pass: <.., false, true> only; unsupported cross shapes run the 4 x 4 kernel
    assert kt.dispatch(kt.FWD, dict(real, Nrows=64, cross=32, psky_complex=-1)) == [
        ('fringe_ant_fwd_cross_kernel<1, 1, false, true>', '')]
    assert kt.dispatch(kt.FWD, dict(real, Nrows=256, cross=128))[1] == ('fringe_ant_fwd_cross_kernel<4, 4, false, false>', '')
    # backward: <= 64 rows the two-tile kernel; the mirror mask is ignored on cross blocks
    assert kt.dispatch(kt.BWD, dict(Nrows=64, cross=0, mirror=1, psky_complex=0, accumulate=1)) == [
        ('fringe_ant_bwd_kernel<false, 2>', 'accumulate=1'), ('fringe_ant_bwd_kernel<false, 2>', 'mirror=1')]
    assert kt.dispatch(kt.BWD, dict(Nrows=65, cross=0, mirror=0, psky_complex=1, accumulate=0)) == [
        ('fringe_ant_bwd_kernel<true, 4>', 'accumulate=0')]
    # pair form: a hub takes the two-tile kernels whatever the row count
    assert kt.dispatch(kt.PBWD, dict(Nrows=20, centre=True, flat=False, accumulate=0)) == [
        ('fringe_pair_bwd_kernel<true, false, 2>', 'accumulate=0')]


@pytest.mark.parametrize('Nt,Nf,P,S_fwd,S_bwd', [(3, 520, 1024, 1, 1), (3, 520, 17024, 2, 3), (2, 7, 17024, 15, 67),
                                                 (1, 1, 98304, 96, 384)])
def test_split_plans(Nt, Nf, P, S_fwd, S_bwd):
    """the pixel splits restated from fwd_split_plan and bwd_split_plan, and the workspace the library sizes
    from the same forward split"""
    from bayeslim_amd import ops
    assert kt.fwd_splits(Nt, Nf, P) == S_fwd
    assert kt.bwd_splits(Nt, Nf, P)[0] == S_bwd
    Nbl = 5
    assert ops.lib.rime_fringe_ant_workspace(Nbl, Nt, Nf, P) == S_fwd * Nbl * Nt * Nf * 8
    assert kt.grid(kt.FWD, Nt, Nf, P) == Nt * Nf * S_fwd and kt.grid(kt.PBWD, Nt, Nf, P) == Nt * Nf * S_bwd


def test_gpu_cases_reach_every_table_row_on_the_host(monkeypatch):
    """the cases of tests/test_fringe_kernels_gpu.py run through ops' launch sequence with a library stand-in that accepts
    every block launch (CPU tensors, nothing computed): each case reaches the rows the table assigns to it, and together
    they reach every row.  The GPU module asserts the same on the real launches."""
    from bayeslim_amd import ops
    real = ops.lib

    class HostOnlyLib:
        """the library's host-side workspace sizes as they are; every other call accepted, nothing launched"""
        def __getattr__(self, name):
            fn = getattr(real, name)
            return fn if 'workspace' in name else (lambda *args: 0)

    fake = kt.LaunchRecorder(HostOnlyLib())
    monkeypatch.setattr(ops, 'lib', fake)
    monkeypatch.setattr(ops, '_require_cuda', lambda *a: None)
    monkeypatch.setattr(ops, '_stream', lambda: ctypes.c_void_p(0))
    reached = set()
    for cid, spec in kt.CASES.items():
        monkeypatch.setattr(ops, 'MIRROR', True)
        monkeypatch.setattr(ops, 'PAIR', spec.get('pair', True))
        monkeypatch.setattr(ops, 'PAIR_CPLX', True)
        monkeypatch.setattr(ops, 'SELF_BLOCKS', True)
        ant, pairs, bl_mp, mp_pairs = kt.build_case(cid)
        antp = torch.as_tensor(ant, dtype=torch.float64)
        blvecs = antp[[b for _, b in pairs]] - antp[[a for a, _ in pairs]]
        Nmp = len(mp_pairs) if mp_pairs else 1
        geom = ops.FringeGeometry(blvecs, torch.zeros(1, 3, 64, dtype=torch.float64), [1.5e8], bl_mp=bl_mp, Nmp=Nmp,
                                  antpos=antp, bl_ants=pairs, mfma=True, group=spec.get('group'), mp_pairs=mp_pairs)
        assert geom.ant is not None, cid
        rows = set()
        for kind in spec.get('psky', ('real',)):
            cplx = kind == 'complex'
            x = torch.zeros((1, Nmp, 1, 1, 64), dtype=torch.complex64 if cplx else torch.float32)
            v = torch.zeros((1, len(pairs), 1, 1), dtype=torch.complex64)
            fake.calls.clear()
            ops._fringe_call_planes(geom, False, x, v, cplx)
            ops._fringe_call_planes(geom, True, x, v, cplx)
            rows |= {row for row, _, _ in fake.rows()}
        mine = {row for row, info in kt.KERNELS.items() if info['case'] == cid}
        assert mine <= rows, (cid, sorted(mine - rows))
        reached |= rows
    assert reached == set(kt.KERNELS), sorted(set(kt.KERNELS) ^ reached)
