"""
The return code of every REJECTED call of the vector-ALU entry points (include/rime_hip.h), as one table -- without a GPU.

These entry points share one host dispatch (with_real, with_bool, as_stream in rime_common.h).  Each row is a
call that returns before anything is launched: the arguments of an acceptable call (BASE) with one or two of them made bad.
Every entry point gets an unknown dtype (7 and -1), each required pointer null, a bad size or flag, and a row with two faults
for every pair of checks whose order matters:

  * dtype with the workspace: rime_chisq_fwd looks at the workspace FIRST (RIME_EWORKSPACE); every other entry point that
    takes one looks at dtype first;
  * dtype with a grid beyond 2^31 - 1 blocks: jones_apply and stokes2coh say RIME_EUNSUPPORTED before they look at dtype;
  * dtype with a null pointer;
  * dtype with the early RIME_OK of an empty call (fft, lstbin, filt, sfb, hmc): dtype is looked at first, so the empty call
    of an unknown dtype is RIME_EINVAL and that of a known one RIME_OK (the only rows that expect success: nothing is
    launched for them either).

The acceptable call itself is never made: the pointers are those of a small host buffer.
"""
import ctypes

import pytest

from bayeslim_amd import _lib

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -4

_BUF = ctypes.create_string_buffer(4096)                             # zeros
PTR = ctypes.addressof(_BUF)
_UNIT = (ctypes.c_double * 3)(1.0, 0.0, 0.0)                         # a barycentric velocity of |v| = c
UNIT = ctypes.addressof(_UNIT)
_KEEP = []


def IP(*vals):
    """a host table of ints, for the arguments declared int* in _lib.SIGNATURES"""
    a = (ctypes.c_int * len(vals))(*vals)
    _KEEP.append(a)
    return a


BIG = 256 * 0x7fffffff + 1                                           # elements of a 1-D grid of 2^31 blocks of 256
NAN = float('nan')
_RC = dict(Nout=1, Nin=1, Nterms=1, Nent=1)
_CP = dict(N=2, Nbl=1, Nout=1, Nt=1, Nf=1, Tm=1, Fm=1, addI=0, prod=0)
_TA = dict(Npp=1, Nbl=1, Nt=1, Nf=4, Nbin=1, Nmem=1)
_FR = dict(mp_offsets_host=IP(0, 5), bl_order=None, Nbl=5, Nt=1, Nf=1, Pstride=64, Nmp=1, Npp=1, psky_complex=0, sign=1,
           freq_uniform_host=0, freq0_host=1e8, dfreq_host=1e6, max_blen_host=0.0, strides_host=None)
_SFB = dict(blocks=PTR, cols=PTR, tiles=PTR, Nblk=1, Ntile=1, B=1, Nlmn=1, Nr=1, Nlm=1)

# arguments in the order of the C declarations; dtype 0 is RIME_F32
BASE = {
    'rime_stokes2coh_fwd': dict(dtype=0, stokesI=PTR, frac=PTR, fs_k=1, fs_r=0, fs_p=0, R=2, P=3, coh=PTR, stream=None),
    'rime_stokes2coh_bwd': dict(dtype=0, gcoh=PTR, frac=PTR, fs_k=1, fs_r=0, fs_p=0, R=2, P=3, gI=PTR, stream=None),
    'rime_jones_apply_fwd': dict(dtype=0, beam_complex=0, J1=PTR, J2=PTR, S=PTR, N=6, Ns=3, out=PTR, stream=None),
    'rime_jones_apply_bwd': dict(dtype=0, beam_complex=0, J1=PTR, J2=PTR, S=PTR, G=PTR, N=6, Ns=3, gJ1=PTR, gJ2=PTR, gS=PTR,
                                 stream=None),
    'rime_chisq_fwd': dict(dtype=0, pred=PTR, data=None, icov=None, N=4, out=PTR, workspace=PTR, workspace_bytes=16384,
                           stream=None),
    'rime_chisq_bwd': dict(dtype=0, pred=PTR, data=None, icov=None, g=PTR, N=4, gpred=PTR, stream=None),
    'rime_apply_cal_fwd': dict(dtype=0, NP=1, diag=1, vis=PTR, gains=PTR, a1=PTR, a2=PTR, Nbl=2, Nt=1, Nf=1, Nant=2, gst_p=1,
                               gst_a=1, gst_t=1, gst_f=1, out=PTR, stream=None),
    'rime_apply_cal_bwd': dict(dtype=0, NP=1, diag=1, vis=PTR, gains=PTR, gout=PTR, a1=PTR, a2=PTR, Nbl=2, Nt=1, Nf=1, Nant=2,
                               gst_p=1, gst_a=1, gst_t=1, gst_f=1, gvis=PTR, d1=PTR, d2=PTR, stream=None),
    'rime_redvis_fwd': dict(dtype=0, NP=1, vis=None, model=PTR, red=PTR, tmap=PTR, Nbl=2, Nt=1, Nf=1, Nred=1, Ntm=1, mst_p=1,
                            mst_r=1, mst_t=1, mst_f=1, sign=1, out=PTR, stream=None),
    'rime_redvis_bwd': dict(dtype=0, NP=1, gout=PTR, goff=PTR, gmem=PTR, toff=PTR, tmem=PTR, Nbl=2, Nt=1, Nf=1, Nred=1, Ntm=1,
                            sign=1, gmodel=PTR, stream=None),
    'rime_vis_timeavg_fwd': dict(dtype=0, data=PTR, wgts=None, cov=None, flags=None, tau=None, tau_by_member=0, freqs=None,
                                 bin_ptr=PTR, members=PTR, bin_ptr_host=IP(0, 1), members_host=IP(0), **_TA, avg=PTR,
                                 sum_w=PTR, avg_cov=None, avg_flag=None, stream=None),
    'rime_vis_timeavg_bwd': dict(dtype=0, gavg=PTR, wgts=None, sum_w=PTR, tau=None, tau_by_member=0, freqs=None, t_ptr=PTR,
                                 t_pos=PTR, pos_bin=PTR, t_ptr_host=IP(0, 1), t_pos_host=IP(0), pos_bin_host=IP(0), **_TA,
                                 gdata=PTR, stream=None),
    'rime_filt_apply': dict(dtype=0, wcplx=0, x=PTR, Wt=PTR, ic=PTR, oc=PTR, base=PTR, tiles=PTR, Ntile=1, Npass=0, Nfilt=1,
                            M=4, K=4, Nx=4, Ny=4, Nlines=1, s=1.0, y=PTR, stream=None),
    'rime_sfb_fwd': dict(dtype=0, cplx=0, params=PTR, g=PTR, **_SFB, out=PTR, stream=None),
    'rime_sfb_bwd': dict(dtype=0, cplx=0, gout=PTR, g=PTR, **_SFB, gparams=PTR, stream=None),
    'rime_interp_gather_fwd': dict(dtype=0, is_complex=0, m=PTR, inds=PTR, wgts=PTR, R=1, Npb=1, P=1, Nnn=1, out=PTR,
                                   out_stride=1, stream=None),
    'rime_interp_scatter_bwd': dict(dtype=0, is_complex=0, goutT=PTR, csr_ptr=PTR, csr_src=PTR, wgts=PTR, R=1, Npb=1, P=1,
                                    Nnn=1, gmT=PTR, stream=None),
    'rime_interp_scatter_rows_bwd': dict(dtype=0, is_complex=0, gout=PTR, gout_stride=1, csr_ptr=PTR, csr_src=None, wgts=PTR,
                                         R=1, Npb=1, gm=PTR, stream=None),
    'rime_beam_sky_fwd': dict(dtype=0, bmapT=PTR, sky=PTR, inds=PTR, wgts=PTR, cut=PTR, R=1, Npb=1, Npix=1, Q=1, Nnn=1,
                              psky=PTR, stream=None),
    # eight time steps: the sky gradient is split in two, whose partial planes need a workspace of 2 x R x Npix reals
    'rime_beam_sky_bwd': dict(dtype=0, gpsky=PTR, bmapT=PTR, sky=PTR, inds=PTR, wgts=PTR, cut=PTR, pos=PTR, R=1, Npb=1,
                              Npix=1, Nt=8, Ps=1, Nnn=1, T1=PTR, gsky=PTR, workspace=PTR, workspace_bytes=8, stream=None),
    'rime_lm_apply': dict(dtype=0, xcplx=0, mcplx=0, out_real=0, x=PTR, M=PTR, m_rs=4, m_ks=1, idx=None, pre=None, post=None,
                          O=1, K=4, K_in=4, R=4, I=1, y=PTR, stream=None),
    'rime_fft_apply': dict(dtype=0, x=PTR, tw=PTR, win=None, win_on_store=0, radix=IP(8), nradix=1, N=8, nlines=1, inverse=0,
                           shift_in=0, shift_out=0, scale=1.0, epilogue=0, start=0.0, df=1.0, y=PTR, stream=None),
    'rime_hmc_step': dict(dtype=0, N=4, q=PTR, p=PTR, g=PTR, eps=None, c=None, kick=0.5, drift=0.5, energy=PTR, workspace=PTR,
                          workspace_bytes=_lib.lib.rime_hmc_workspace(4), stream=None),
    'rime_hmat_apply': dict(dtype=0, tiles=PTR, ntiles=1, ranges=PTR, tile_ids=PTR, stage_first=IP(0, 1), nstages=1,
                            scratch_rows=4, x=PTR, y=PTR, nrhs=1, scalar=1.0, accumulate=0, workspace=PTR, workspace_bytes=16,
                            stream=None),
    'rime_lbfgs_dots': dict(dtype=0, s_rows=PTR, y_rows=PTR, m=1, N=4, v=PTR, d=None, k=-1, out=PTR, workspace=PTR,
                            workspace_bytes=_lib.lib.rime_lbfgs_workspace(1, 4), stream=None),
    'rime_lbfgs_combine': dict(dtype=0, s_rows=PTR, y_rows=PTR, m=1, N=4, v=PTR, d=None, a=PTR, b=PTR, gamma=1.0, r=PTR,
                               stream=None),
    # prod 0 = RIME_COUPLING_BOTH: the forward keeps E V, one (N, N, Nt, Nf) complex matrix of 32 bytes, in the workspace
    'rime_coupling_fwd': dict(dtype=0, x=PTR, dly=None, data=PTR, tab=PTR, otab=PTR, **_CP, out=PTR, workspace=PTR,
                              workspace_bytes=32, stream=None),
    'rime_coupling_bwd': dict(dtype=0, x=PTR, dly=None, data=PTR, gout=PTR, tab=PTR, otab=PTR, ftab=PTR, **_CP, gdata=PTR,
                              gx=PTR, workspace=PTR, workspace_bytes=64, stream=None),
    'rime_coupling_expand': dict(dtype=0, x=PTR, dly=None, N=2, Nt=1, Nf=1, Tm=1, Fm=1, addI=0, e=PTR, stream=None),
    # two times of one coupling matrix: the gradient is summed over them from a workspace of 64 bytes
    'rime_coupling_expand_bwd': dict(dtype=0, x=PTR, dly=None, ge=PTR, N=2, Nt=2, Nf=1, Tm=1, Fm=1, gx=PTR, workspace=PTR,
                                     workspace_bytes=64, stream=None),
    'rime_redcoupling_fwd': dict(dtype=0, x=PTR, dly=None, data=PTR, ent=PTR, roff=PTR, **_RC, Nt=1, Nf=1, Tm=1, Fm=1, out=PTR,
                                 stream=None),
    'rime_redcoupling_bwd_data': dict(dtype=0, x=PTR, dly=None, gout=PTR, ent=PTR, coff=PTR, cmem=PTR, **_RC, Nt=1, Nf=1, Tm=1,
                                      Fm=1, gdata=PTR, stream=None),
    'rime_redcoupling_bwd_coupling': dict(dtype=0, x=PTR, dly=None, data=PTR, gout=PTR, ent=PTR, toff=PTR, tmem=PTR,
                                          segterm=PTR, segstart=PTR, tsoff=PTR, **_RC, Nmem=1, Nseg=1, seg=1, Nt=1, Nf=1, Tm=1,
                                          Fm=1, gx=PTR, workspace=PTR, workspace_bytes=8, stream=None),
    'rime_fringe_sum_fwd': dict(dtype=0, blvecs=PTR, sdir=PTR, freqs=PTR, psky=PTR, **_FR, vis=PTR, workspace=PTR,
                                workspace_bytes=1 << 40, stream=None),
    'rime_fringe_sum_bwd': dict(dtype=0, blvecs=PTR, sdir=PTR, freqs=PTR, gvis=PTR, **_FR, gpsky=PTR, workspace=PTR,
                                workspace_bytes=1 << 40, stream=None),
    'rime_gen_fringe': dict(dtype=0, blvecs=PTR, sdir=PTR, freqs=PTR, Nbl=1, Nf=1, P=1, sdir_stride=1, sign=1, out=PTR,
                            stream=None),
    'rime_eq2top': dict(ra_deg=PTR, dec_deg=PTR, N=1, M_host=PTR, vbary_host=PTR, vdiurnal=0.0, zen_deg=PTR, az_deg=PTR,
                        stream=None),
}

# pointers that may be null in an acceptable call, besides those BASE leaves null
OPTIONAL = {'rime_redvis_fwd': ['tmap'], 'rime_hmc_step': ['energy'], 'rime_vis_timeavg_fwd': ['data', 'sum_w'], 'rime_fringe_sum_fwd': ['workspace'],
            'rime_fringe_sum_bwd': ['workspace'], 'rime_coupling_bwd': ['gdata', 'gx', 'ftab']}
WORKSPACE = [e for e in BASE if 'workspace' in BASE[e] and not e.startswith('rime_fringe_sum')]

# one bad size or flag each (more for the entry points with checks of several kinds); all RIME_EINVAL
BAD = {
    'rime_stokes2coh_fwd': [dict(R=0), dict(fs_k=-1)],
    'rime_stokes2coh_bwd': [dict(P=0), dict(fs_p=-1)],
    'rime_jones_apply_fwd': [dict(Ns=4), dict(N=0)],
    'rime_jones_apply_bwd': [dict(Ns=4), dict(Ns=0)],
    'rime_chisq_fwd': [dict(N=0)],
    'rime_chisq_bwd': [dict(N=0)],
    'rime_apply_cal_fwd': [dict(NP=3), dict(Nbl=0)],
    'rime_apply_cal_bwd': [dict(NP=0), dict(Nant=0)],
    'rime_redvis_fwd': [dict(sign=0), dict(mst_p=-1), dict(tmap=None, Ntm=2), dict(NP=3)],
    'rime_redvis_bwd': [dict(sign=2), dict(Nred=0)],
    'rime_vis_timeavg_fwd': [dict(tau_by_member=2), dict(Npp=-1), dict(cov=PTR), dict(tau=PTR), dict(bin_ptr_host=IP(0, 2)),
                             dict(members_host=IP(1))],
    'rime_vis_timeavg_bwd': [dict(tau_by_member=-1), dict(Nf=-1), dict(tau=PTR), dict(t_ptr_host=IP(1, 1)),
                             dict(pos_bin_host=IP(1))],
    'rime_filt_apply': [dict(wcplx=2), dict(s=2.0), dict(Npass=2), dict(Npass=1, Nx=5), dict(M=0)],
    'rime_sfb_fwd': [dict(cplx=2), dict(Nr=0), dict(Nblk=0)],
    'rime_sfb_bwd': [dict(cplx=-1), dict(Nlm=0), dict(Nblk=0)],
    'rime_interp_gather_fwd': [dict(out_stride=0), dict(R=0)],
    'rime_interp_scatter_bwd': [dict(Nnn=0), dict(Npb=0)],
    'rime_interp_scatter_rows_bwd': [dict(gout_stride=0), dict(R=0)],
    'rime_beam_sky_fwd': [dict(Q=0), dict(Nnn=0)],
    'rime_beam_sky_bwd': [dict(Ps=0), dict(Nt=0)],
    'rime_lm_apply': [dict(out_real=1), dict(K_in=3), dict(m_rs=0), dict(xcplx=2), dict(idx=PTR, K_in=0)],
    'rime_fft_apply': [dict(N=0), dict(shift_in=8), dict(radix=IP(4)), dict(scale=NAN), dict(epilogue=-1),
                       dict(inverse=2), dict(nlines=-1)],
    'rime_hmc_step': [dict(N=-1), dict(kick=NAN), dict(kick=1e-60), dict(drift=1e-60), dict(drift=NAN), dict(N=(1 << 62)), dict(kick=-1e-60),
                      dict(drift=0.0, q=None, kick=NAN), dict(kick=0.0, g=None, drift=-1e-60)],
    'rime_hmat_apply': [dict(nstages=0), dict(nrhs=0), dict(stage_first=IP(1, 0)), dict(stage_first=IP(-1, 0))],
    'rime_lbfgs_dots': [dict(k=1), dict(m=0), dict(N=0)],
    'rime_lbfgs_combine': [dict(m=0), dict(N=0)],
    'rime_coupling_fwd': [dict(prod=3), dict(addI=2), dict(Tm=2), dict(Nbl=0)],
    'rime_coupling_bwd': [dict(prod=-1), dict(addI=-1), dict(Fm=2), dict(gdata=None, gx=None), dict(ftab=None)],
    'rime_coupling_expand': [dict(addI=2), dict(N=0)],
    'rime_coupling_expand_bwd': [dict(Tm=3), dict(Nf=0)],
    'rime_redcoupling_fwd': [dict(Tm=2), dict(Nterms=0)],
    'rime_redcoupling_bwd_data': [dict(Fm=2), dict(Nin=0)],
    'rime_redcoupling_bwd_coupling': [dict(seg=0), dict(Nseg=2), dict(Nmem=0), dict(Nseg=0)],
    'rime_fringe_sum_fwd': [dict(Pstride=63), dict(Npp=3), dict(sign=0), dict(mp_offsets_host=IP(0, 4)), dict(Nmp=0)],
    'rime_fringe_sum_bwd': [dict(Pstride=0), dict(Npp=3), dict(sign=2), dict(mp_offsets_host=IP(1, 5)), dict(Nbl=0)],
    'rime_gen_fringe': [dict(sdir_stride=0), dict(sign=0)],
    'rime_eq2top': [dict(N=-1), dict(vbary_host=UNIT)],
}

# a 1-D grid of 2^31 blocks: refused before dtype is looked at
TOO_LONG = {'rime_stokes2coh_fwd': dict(R=BIG, P=1), 'rime_stokes2coh_bwd': dict(R=BIG, P=1),
            'rime_jones_apply_fwd': dict(N=BIG, Ns=BIG), 'rime_jones_apply_bwd': dict(N=BIG, Ns=BIG)}

# calls with nothing to write: RIME_OK without a launch, but only after dtype has been looked at
EMPTY = {'rime_fft_apply': [dict(nlines=0)], 'rime_vis_timeavg_fwd': [dict(Npp=0), dict(Nbin=0, Nmem=0, bin_ptr_host=IP(0))],
         'rime_vis_timeavg_bwd': [dict(Nbl=0)], 'rime_filt_apply': [dict(Ntile=0), dict(Nlines=0), dict(Ntile=0, x=None)],
         'rime_sfb_fwd': [dict(Ntile=0), dict(B=0)], 'rime_sfb_bwd': [dict(Ntile=0), dict(B=0, gout=None)],
         'rime_hmc_step': [dict(kick=0.0, drift=0.0, energy=None), dict(kick=0.0, drift=-0.0, energy=None, q=None, g=None, workspace=None)]}


def _required(entry):
    """the pointers of BASE (device buffers and host tables) that an acceptable call cannot leave null"""
    opt = OPTIONAL.get(entry, []) + ['workspace']
    return [k for k, v in BASE[entry].items() if (v == PTR or isinstance(v, ctypes.Array)) and k not in opt]


def _rows():
    rows = []

    def add(entry, code, **bad):
        rows.append((entry, bad, code))

    for e in BASE:
        typed = 'dtype' in BASE[e]
        if typed:
            add(e, EINVAL, dtype=7)
            add(e, EINVAL, dtype=-1)
        for name in _required(e):                                    # null pointers, one at a time
            add(e, EINVAL, **{name: None})
        if typed:
            add(e, EINVAL, dtype=7, **{_required(e)[0]: None})       # ... and with an unknown dtype
        for bad in BAD[e]:
            add(e, EINVAL, **bad)
        if typed:
            add(e, EINVAL, dtype=7, **BAD[e][0])
    for e, big in TOO_LONG.items():
        add(e, EUNSUPPORTED, **big)
        add(e, EUNSUPPORTED, dtype=7, **big)
        add(e, EUNSUPPORTED, dtype=-1, **big)
        add(e, EINVAL, **big, **{_required(e)[0]: None})             # a null pointer ahead of the grid
    for e in WORKSPACE:                                              # no workspace, or one a byte short
        first = EWORKSPACE if e == 'rime_chisq_fwd' else EINVAL
        for short in (dict(workspace=None), dict(workspace_bytes=BASE[e]['workspace_bytes'] - 1)):
            if e == 'rime_beam_sky_bwd' and 'workspace' in short:
                continue                                             # without a workspace it walks the time steps in one go
            add(e, EWORKSPACE, **short)
            add(e, first, dtype=7, **short)
            add(e, first, dtype=-1, **short)
            add(e, EINVAL, **short, **BAD[e][0])                     # sizes and flags ahead of the workspace
    add('rime_hmc_step', EWORKSPACE, kick=1e-60, workspace=None)     # ... but the step that underflows in float32 after it
    add('rime_hmc_step', EINVAL, dtype=7, kick=1e-60)
    add('rime_hmc_step', EINVAL, kick=0.0, drift=0.0, energy=None, N=-1)       # nothing to do is RIME_OK only after every check
    add('rime_hmc_step', EINVAL, kick=0.0, drift=0.0, energy=None, p=None)
    add('rime_hmc_step', EWORKSPACE, kick=0.0, drift=0.0, workspace_bytes=0)
    add('rime_beam_sky_bwd', EINVAL, dtype=7, workspace=None, workspace_bytes=0)
    # the generic fringe sum: a full-polarisation complex psky of two feeds is refused before dtype is looked at; the
    # workspace is looked at after it (one (t, f) row of 2^20 pixels is split, so that it needs one)
    for e in ('rime_fringe_sum_fwd', 'rime_fringe_sum_bwd'):
        add(e, EUNSUPPORTED, Npp=2, psky_complex=1)
        add(e, EUNSUPPORTED, dtype=7, Npp=2, psky_complex=1)
        add(e, EUNSUPPORTED, Npp=2, psky_complex=1, sign=0)
        add(e, EINVAL, Npp=2, psky_complex=1, Pstride=63)
    add('rime_fringe_sum_fwd', EWORKSPACE, Pstride=1 << 20, workspace_bytes=0)
    add('rime_fringe_sum_fwd', EINVAL, dtype=7, Pstride=1 << 20, workspace_bytes=0)
    add('rime_fringe_sum_bwd', EWORKSPACE, Nbl=4096, mp_offsets_host=IP(0, 4096), workspace_bytes=0)
    add('rime_fringe_sum_bwd', EINVAL, dtype=-1, Nbl=4096, mp_offsets_host=IP(0, 4096), workspace_bytes=0)
    for e, empties in EMPTY.items():
        for empty in empties:
            add(e, OK, **empty)
            add(e, OK, dtype=1, **empty)
            add(e, EINVAL, dtype=7, **empty)
            add(e, EINVAL, dtype=-1, **empty)
    add('rime_eq2top', OK, N=0)
    return rows


ROWS = _rows()


def _show(v):
    return '%d' % v if isinstance(v, int) else 'tab%s' % '.'.join(map(str, v)) if isinstance(v, ctypes.Array) else str(v)


def _id(row):
    entry, bad, code = row
    return entry[len('rime_'):] + '-' + '-'.join('%s=%s' % (k, 'ptr' if v == PTR else 'unit' if v == UNIT else _show(v)) for k, v in bad.items())


def test_table_is_complete():
    """every row changes an argument of its entry point, every entry point has as many arguments as its C declaration, the
    rows that expect success are those of EMPTY and the empty rime_eq2top, and the shapes chosen to need a workspace need one"""
    assert {e for e, _, _ in ROWS} == set(BASE) == set(BAD)
    for entry, bad, code in ROWS:
        assert code in (OK, EINVAL, EWORKSPACE, EUNSUPPORTED)
        assert bad and set(bad) <= set(BASE[entry]), (entry, bad)
        assert len(BASE[entry]) == len(_lib.SIGNATURES[entry][1]), entry
        if code == OK:
            assert bad.get('dtype', 0) in (0, 1) and (entry in EMPTY or entry == 'rime_eq2top')
    assert len({_id(r) for r in ROWS}) == len(ROWS)
    L = _lib.lib
    assert L.rime_chisq_workspace() == BASE['rime_chisq_fwd']['workspace_bytes']
    assert L.rime_beam_sky_bwd_workspace(0, 1, 1, 8) == BASE['rime_beam_sky_bwd']['workspace_bytes']
    assert 0 < BASE['rime_hmc_step']['workspace_bytes'] and 0 < BASE['rime_lbfgs_dots']['workspace_bytes']
    assert L.rime_hmat_workspace(0, 4, 1) == BASE['rime_hmat_apply']['workspace_bytes']
    assert L.rime_coupling_workspace(0, 2, 1, 1, 1, 1, 0, 0) == BASE['rime_coupling_fwd']['workspace_bytes']
    assert L.rime_coupling_workspace(0, 2, 1, 1, 1, 1, 0, 1) == BASE['rime_coupling_bwd']['workspace_bytes']
    assert L.rime_coupling_workspace(0, 2, 2, 1, 1, 1, 0, 2) == BASE['rime_coupling_expand_bwd']['workspace_bytes']
    assert L.rime_redcoupling_workspace(0, 1, 1, 1) == BASE['rime_redcoupling_bwd_coupling']['workspace_bytes']
    assert L.rime_fringe_sum_workspace(0, 5, 1, 1, 1 << 20, 1, 1, 0, 0) > 0
    assert L.rime_fringe_sum_workspace(0, 4096, 1, 1, 64, 1, 1, 0, 1) > 0


@pytest.mark.parametrize('row', ROWS, ids=_id)
def test_rejected_call_returns_its_code(row, monkeypatch):
    monkeypatch.delenv('RIME_SKYGRAD_SPLITS', raising=False)         # a lab switch that would change the splits of BASE
    entry, bad, code = row
    args = dict(BASE[entry], **bad)
    assert getattr(_lib.lib, entry)(*args.values()) == code
