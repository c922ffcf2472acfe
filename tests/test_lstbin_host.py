"""
Host-side checks of the LST alignment stage (csrc/lstbin.hip, ops.TimeAvgPlan / vis_timeavg, telescope_model.rephase_tau,
VisData.lst_rephase / time_nn_interp / time_average): nothing here launches a kernel.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lstbin_common as lc
import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kind,name', [('rephase', n) for n in lc.REPHASE_CASES] + lc.fixture_cases())
def test_restatement_reproduces_the_fixture(kind, name):
    """the float64 numpy restatement the GPU tests compare against, fed with the recorded inputs, gives the reference's
    recorded outputs within FACTOR x the recorded constant; and the constant is the one this fixture gives"""
    worst = lc.compare(lc.restate_case(kind, name), lc.recorded(kind, name), lambda k: lc.FACTOR * lc.RESTATEMENT)
    assert all(v <= lc.RESTATEMENT * 1.01 for v in worst.values()), worst


def test_tau_closed_forms_and_records():
    from bayeslim_amd import telescope_model as tm
    bv = lc.fix_blvecs()
    assert np.abs(tm.rephase_tau(np.zeros(4), lc.FIX_LAT, bv).numpy()).max() == 0.0
    assert np.abs(tm.rephase_tau(0.0, 12.0, bv).numpy()).max() == 0.0
    dl = np.linspace(-1.0, 1.0, 9)
    ew = np.array([[14.6, 0.0, 0.0], [-73.0, 0.0, 0.0]])
    got = tm.rephase_tau(dl, 0.0, ew).numpy()
    want = -ew[:, :1] * np.sin(dl)[None] / lc.C_LIGHT
    assert got.shape == (2, 9) and np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    for name, (dlst, lat) in lc.REPHASE_CASES.items():
        rec = lc.golden()['rephase_%s_tau' % name]
        got = tm.rephase_tau(torch.as_tensor(dlst), lat, torch.as_tensor(bv)).numpy()
        assert got.shape == rec.shape and got.dtype == np.float64
        assert np.abs(got - rec).max() <= lc.TAU_RTOL * max(np.abs(rec).max(), 1e-300), name


def test_bin_table_and_its_transpose():
    from bayeslim_amd import ops
    from bayeslim_amd.dataset import time_bins
    for name, bins in list(lc.BIN_TABLES.items()) + [('empty', [[0, 1], [], [4], []])]:
        plan = ops.TimeAvgPlan(bins, lc.NT)
        ptr, mem = lc.csr(bins)
        assert plan.bin_ptr.dtype == np.int32 and (plan.bin_ptr == ptr).all() and (plan.members == mem).all(), name
        assert plan.Nbin == len(bins) and plan.Nmem == len(mem)
        tr = lc.transpose(bins, lc.NT)
        assert plan.t_ptr[0] == 0 and plan.t_ptr[-1] == plan.Nmem
        for t in range(lc.NT):
            pos = plan.t_pos[plan.t_ptr[t]:plan.t_ptr[t + 1]].tolist()
            assert pos == [m for m, _ in tr[t]], (name, t)
            assert plan.pos_bin[pos].tolist() == [k for _, k in tr[t]], (name, t)
    assert ops.TimeAvgPlan(lc.BIN_TABLES['dropped'], lc.NT).t_ptr[4:6].tolist() == [4, 4]      # time 4: in no bin
    with pytest.raises(ValueError):
        ops.TimeAvgPlan([[0, 7]], 7)
    with pytest.raises(ValueError):
        ops.TimeAvgPlan([[-1]], 7)
    # time_average's rule: a time listed twice goes to the last entry, an unlisted time to none, an empty entry stays
    bins, index = time_bins([[0, 1, 2], [2, 3], [], torch.tensor([5])], 7)
    assert [b.tolist() for b in bins] == [[0, 1], [2, 3], [], [5]] and index.tolist() == [0, 0, 1, 1, 4, 3, 4]


def test_nearest_lst_selection_across_the_wrap():
    from bayeslim_amd.dataset import nearest_lst
    G = lc.golden()
    for name, (pol, jd0, offs, rephase) in lc.NN_CASES.items():
        times, lsts = G[name + '_times'], G[name + '_lsts']
        keep = lsts.copy()
        t_idx, dLST = nearest_lst(lsts, np.deg2rad(lc.jd2lst(times, lc.FIX_LON)))
        assert (lsts == keep).all()                                          # the caller's array is left alone
        assert np.abs(times[t_idx] - G[name + '_out_times']).max() == 0.0, name
        ri, rd = lc.nearest(lsts, np.deg2rad(lc.jd2lst(times, lc.FIX_LON)))
        assert (t_idx == ri).all() and np.abs(dLST - rd).max() <= 1e-15
        assert np.abs(dLST).max() <= 0.51 * lc._STEP, name                   # never further than half an integration
    sl = np.deg2rad(lc.jd2lst(G['nn_wrap_times'], lc.FIX_LON))
    assert sl[-1] < sl[0] and G['nn_wrap_lsts'][-1] < G['nn_wrap_lsts'][0]
    # targets that start after the wrap while the data start before it
    t_idx, dLST = nearest_lst(np.array([0.01, 0.02]), np.array([6.27, 6.28, 0.007, 0.017, 0.027]))
    assert t_idx.tolist() == [2, 3] and np.allclose(dLST, [0.003, 0.003])


def _fwd_args(**kw):
    one = ctypes.c_void_p(8)          # non-null dummy; never dereferenced on a rejected call
    ptr = (ctypes.c_int * 4)(0, 1, 3, 7)
    mem = (ctypes.c_int * 7)(0, 1, 2, 3, 4, 5, 6)
    a = dict(dtype=0, data=one, wgts=None, cov=None, flags=None, tau=None, by_member=0, freqs=None, bin_ptr=one, members=one,
             bin_ptr_host=ptr, members_host=mem, Npp=1, Nbl=3, Nt=7, Nf=5, Nbin=3, Nmem=7, avg=one, sum_w=None, avg_cov=None,
             avg_flag=None, stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(**kw):
    one = ctypes.c_void_p(8)
    tptr = (ctypes.c_int * 8)(0, 1, 2, 3, 4, 5, 6, 7)
    tpos = (ctypes.c_int * 7)(0, 1, 2, 3, 4, 5, 6)
    pbin = (ctypes.c_int * 7)(0, 1, 1, 2, 2, 2, 2)
    a = dict(dtype=0, gavg=one, wgts=None, sum_w=one, tau=None, by_member=0, freqs=None, t_ptr=one, t_pos=one, pos_bin=one,
             t_ptr_host=tptr, t_pos_host=tpos, pos_bin_host=pbin, Npp=1, Nbl=3, Nt=7, Nf=5, Nbin=3, Nmem=7, gdata=one, stream=None)
    a.update(kw)
    return list(a.values())


def test_rejected_calls_return_einval_without_a_launch():
    """validation precedes every HIP call, so it runs without a GPU: the pointers handed over are never followed"""
    from bayeslim_amd._lib import lib
    one = ctypes.c_void_p(8)
    I = lambda *v: (ctypes.c_int * len(v))(*v)
    bad_fwd = [dict(dtype=7), dict(avg=None), dict(bin_ptr=None), dict(members=None), dict(bin_ptr_host=None),
               dict(members_host=None), dict(Npp=-1), dict(Nbl=-1), dict(Nt=-1), dict(Nf=-1), dict(Nbin=-1), dict(Nmem=-1),
               dict(by_member=2), dict(tau=one), dict(cov=one), dict(avg_cov=one), dict(flags=one), dict(avg_flag=one),
               dict(bin_ptr_host=I(0, 3, 1, 7)),                            # decreasing
               dict(bin_ptr_host=I(1, 1, 3, 7)),                            # does not start at 0
               dict(bin_ptr_host=I(0, 1, 3, 6)),                            # does not end at Nmem
               dict(members_host=I(0, 1, 2, 3, 4, 5, 7)),                   # member = Nt
               dict(members_host=I(0, -1, 2, 3, 4, 5, 6))]
    for kw in bad_fwd:
        assert lib.rime_vis_timeavg_fwd(*_fwd_args(**kw)) == -1, kw
    bad_bwd = [dict(dtype=-1), dict(gavg=None), dict(sum_w=None), dict(gdata=None), dict(t_ptr=None), dict(t_pos=None),
               dict(pos_bin=None), dict(t_ptr_host=None), dict(t_pos_host=None), dict(pos_bin_host=None), dict(Nt=-1),
               dict(Nbin=-2), dict(by_member=-1), dict(tau=one),
               dict(t_ptr_host=I(0, 1, 2, 3, 4, 3, 6, 7)), dict(t_pos_host=I(0, 1, 2, 3, 4, 5, 7)),
               dict(pos_bin_host=I(0, 1, 1, 2, 2, 2, 3))]
    for kw in bad_bwd:
        assert lib.rime_vis_timeavg_bwd(*_bwd_args(**kw)) == -1, kw
    # an empty output is no error and no launch
    assert lib.rime_vis_timeavg_fwd(*_fwd_args(Nf=0)) == 0
    assert lib.rime_vis_timeavg_bwd(*_bwd_args(Npp=0)) == 0


def _cpu_vd(with_meta=True):
    from bayeslim_amd import dataset, telescope_model, utils
    G = lc.golden()
    vd = dataset.VisData()
    vd.setup_meta(telescope=telescope_model.TelescopeModel((lc.FIX_LON, lc.FIX_LAT)),
                  antpos=utils.AntposDict(lc.FIX_ANTS, torch.as_tensor(np.asarray(lc.FIX_ANTVECS))))
    vd.setup_data(lc.FIX_BLS, lc.fix_times(lc.FIX_JD0), torch.as_tensor(lc.FIX_FREQS), pol='ee',
                  data=torch.as_tensor(G['lstr_scalar_data']))
    return vd


def test_cpu_tensors_raise_the_no_cpu_error():
    from bayeslim_amd import ops, telescope_model
    msg = 'no CPU implementation'
    data = torch.zeros(1, 3, 7, 5, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match=msg):
        ops.vis_timeavg(data, ops.TimeAvgPlan(lc.BIN_TABLES['full'], 7))
    with pytest.raises(RuntimeError, match=msg):
        telescope_model.vis_rephase(0.01, lc.FIX_LAT, lc.fix_blvecs(), torch.as_tensor(lc.FIX_FREQS))
    with pytest.raises(RuntimeError, match=msg):
        _cpu_vd().lst_rephase(dLST=0.01)
    with pytest.raises(RuntimeError, match=msg):
        _cpu_vd().time_average(time_inds=[[0, 1], [2, 3]])
    with pytest.raises(RuntimeError, match=msg):
        _cpu_vd().time_nn_interp(np.deg2rad(lc.jd2lst(lc.fix_times(lc.FIX_JD0)[1:3], lc.FIX_LON)))


def test_kernels_use_no_scratch_and_sixteen_byte_accesses():
    """the gfx950 assembly of this build: eight kernels (dtype x 16-byte / element form), none with a private segment, and 16-byte loads and stores present"""
    asm, kernels, sizes = kernel_asm.read('lstbin')
    assert len(kernels) == 8 and all('vis_timeavg' in k for k in kernels), kernels
    assert sizes == [0] * 8, sizes
    assert not re.findall(r'^\s*scratch_(?:load|store)', asm, flags=re.M)
    assert 'global_load_dwordx4' in asm and 'global_store_dwordx4' in asm
    assert 'atomic' not in asm


def test_layout_constants_match_the_source():
    src = open(os.path.join(ROOT, 'bayeslim_amd', 'csrc', 'lstbin.hip')).read()
    assert re.search(r'TA_THREADS = 256, TA_BYTES = 16\b', src)
    assert lc.LANE_F == {'f32': 16 // 4, 'f64': 16 // 8} and lc.GROUP_F == {'f32': 1024, 'f64': 512}
    assert lc.NF == {'f32': [1, 3, 4, 5, 1023, 1024, 1025], 'f64': [1, 2, 3, 511, 512, 513]}
