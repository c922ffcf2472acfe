"""
Gain application on the GPU: the post-RIME calibration step of the forward model, mirroring
calibration.apply_cal / _apply_cal (calibration.py:2330-2487) -- SURVEY section 8(f) item 3.  The
products of complex visibilities with Jones-type gains run in the fused HIP kernels behind
ops.apply_cal (one pass over the visibility tensor, forward and backward); there is no CPU
implementation.  The other branches of the reference function are small-tensor or elementwise
arithmetic and stay torch ops on the GPU: `undo` inverts the (small) gain tensor first (1-pol / 2-pol:
reciprocal of the diagonal, linalg.diag_inv; 4-pol: the 2 x 2 inverse per antenna, time and channel --
the reference's `torch.pinv` call at :2441 does not exist in torch, so that branch cannot run there),
`vis_type='dly'` adds delay differences, `cov` propagates a variance tensor with |g1 g2*|^2.

`JonesModel` (calibration.py:416-742) is the module that follows RIME in a forward-model chain: parameters ->
`JonesResponse` (calibration.py:745-875: complex / amplitude / phase / delay / slope gain types, optional linear
bases over time and frequency) -> complex gains -> `_apply_cal` on the fused kernels, with the reference-antenna
phase convention (`rephase_to_refant`, :2490-2608) and the time index cache for minibatches (`IndexCache`, :291-413).

Redundant calibration: `RedVisModel` (one visibility per redundant group, calibration.py:877-1053) and `VisModel` (one per
baseline, :1056-1209) add their model to the input VisData through ops.redvis -- the group gather, the time selection of a
minibatch and the add in one pass, and in the backward pass a segmented, fixed-order reduction in place of the atomic
scatter-add that autograd gives the reference's index_select, so the gradient of the model is bit-identical from run to run.
The degeneracy tools (`compute_redcal_degen`, `redcal_degen_gains`, `remove_redcal_degen`, `compute_redcal_degen_vis`,
`redcal_degen_vis`, :2611-2915) are small dense torch arithmetic on whatever device their input is on (CPU included), and
BaseResponse.setup_projection(abs_amp_gain=, phs_slope_gain=, wgts_gain=) projects them out of the gains through
remove_redcal_degen.  `vis2JonesModel` / `vis2RedVisModel` (:2918-2983) build vanilla models from a VisData.
The CalData export is outside the hot path and not built.

Mutual coupling: `VisCoupling` (:1258-1586) applies Vc = E V E^H, E = I + X o D, between the redundant-visibility and the
gain stage through ops.coupling_apply, one batched complex product kernel that reads the visibility matrix from the data through
an index table, builds E on the fly and writes only the baselines of the output.  `RedVisCoupling` (:1588-2115) is the form
fitted on a redundant array, Vc = A(eps) Vr + B(eps) conj(Vr) with one coefficient per coupling vector: ops.redcoupling_apply
sums the non-zero first- and second-order terms from a flat entry list instead of the reference's two dense
(Nbls_out, Nbls_in, Ntimes, Nfreqs) matrices; `gen_coupling_terms`, `configure_coupling_matrix_singlepath`, `cut_bl` and
`CouplingInflate` (:2118-2175, 3047-3400) are its host side.

Partly redundant arrays: `PartialRedVisInflate` (:2178-2344) mixes redundant model visibilities onto the physical baselines
through a sparse matrix with one learnable real number per entry, on ops.partred_inflate: one pass forward and two reductions
in a fixed order backward, in place of the CSR matrix, the transposed copy and the two torch.sparse.mm calls of the reference.
"""
import copy

import numpy as np
import torch

from . import dataset, ops, telescope_model, utils


def _index_tensor(idx, device):
    if torch.is_tensor(idx) and idx.dtype == torch.int32 and idx.device == device:
        return idx
    return torch.as_tensor(idx, device=device).to(torch.int32).contiguous()


def _require_gpu(data):
    if not data.is_cuda:
        raise RuntimeError('bayeslim_amd.calibration needs tensors on the GPU (no CPU implementation)')


def _invert_gains(gains, polmode, vis_type):
    """the `undo` branch (calibration.py:2430-2443) without the per-antenna Python loop"""
    if polmode in ('1pol', '2pol'):
        if vis_type == 'dly':
            return -gains
        if gains.shape[0] == 1:
            return 1 / gains
        inv = torch.zeros_like(gains)                      # linalg.diag_inv: off-diagonals dropped
        inv[0, 0] = 1 / gains[0, 0]
        inv[1, 1] = 1 / gains[1, 1]
        return inv
    assert vis_type == 'com', 'must have complex vis_type for 4pol mode'
    a, b, c, d = gains[0, 0], gains[0, 1], gains[1, 0], gains[1, 1]
    det = a * d - b * c
    return torch.stack([torch.stack([d / det, -b / det]), torch.stack([-c / det, a / det])])


def _apply_cal(vis, gains, g1_idx, g2_idx, cal_2pol=False, cov=None, vis_type='com', undo=False, inplace=False):
    """
    vis (Npol, Npol, Nbl, Ntimes, Nfreqs); gains (Npol, Npol, Nant, Ntimes | 1, Nfreqs | 1);
    g1_idx / g2_idx: len-Nbl indices into the antenna axis of gains for the two antennas of each
    baseline (int32 GPU tensors are used as they are -- build them once; anything else is converted per
    call).  Returns (new_vis, new_cov) like the reference (calibration.py:2412-2487).
    """
    assert vis.shape[:2] == gains.shape[:2], "vis and gains must have same Npols"
    _require_gpu(vis)
    polmode = '1pol' if vis.shape[:2] == (1, 1) else '4pol'
    if cal_2pol and polmode == '4pol':
        polmode = '2pol'
    if undo:
        gains = _invert_gains(gains, polmode, vis_type)
    a1 = _index_tensor(g1_idx, vis.device)
    a2 = _index_tensor(g2_idx, vis.device)
    cov_out = cov
    if vis_type == 'dly':
        assert polmode in ('1pol', '2pol')
        # float delays: V_out = V + tau_1 - tau_2 (:2476)
        return vis + gains.index_select(2, a1.long()) - gains.index_select(2, a2.long()), cov_out
    assert vis_type == 'com'
    # inplace: the reference rebinds its output for complex visibilities, so the flag never changes vis there
    vout = ops.apply_cal(vis, gains.to(vis.dtype) if gains.dtype != vis.dtype else gains, a1, a2,
                         diag=(polmode == '2pol'))
    if cov is not None:
        # variance of the same shape as vis, 1-pol / 2-pol only: cov * |g1 g2*|^2 on the diagonal (:2466-2471)
        assert polmode in ('1pol', '2pol'), 'covariance propagation: 1pol or 2pol mode'
        G = gains.index_select(2, a1.long()) * gains.index_select(2, a2.long()).conj()
        GG = (G * G.conj()).real if torch.is_complex(G) else G * G
        cov_out = torch.zeros_like(cov)
        for p in range(cov.shape[0]):
            cov_out[p, p] = GG[p, p] * cov[p, p]
    return vout, cov_out


def apply_cal(vis, bls, gains, ants, cal_2pol=False, cov=None, vis_type='com', undo=False, inplace=False):
    """
    calibration.apply_cal (calibration.py:2330-2410): bls list of (ant1, ant2), ants list of antenna
    numbers along gains' antenna axis.  Builds the index tensors and calls _apply_cal.
    """
    where = {a: i for i, a in enumerate(ants)}
    g1_idx = torch.as_tensor([where[bl[0]] for bl in bls], dtype=torch.int32, device=vis.device)
    g2_idx = torch.as_tensor([where[bl[1]] for bl in bls], dtype=torch.int32, device=vis.device)
    return _apply_cal(vis, gains, g1_idx, g2_idx, cal_2pol=cal_2pol, cov=cov, vis_type=vis_type,
                      undo=undo, inplace=inplace)


# ---------------------------------------------------------------------------------------
# parameter <-> complex gain conversions (calibration.py:215-288)
# ---------------------------------------------------------------------------------------
def params2complex(params, param_type):
    if param_type == 'real':
        return params + 0j
    if param_type == 'amp':
        return torch.exp(params) + 0j
    if param_type == 'phs':
        return torch.exp(1j * params)
    if param_type == 'amp_phs':
        return torch.exp(params[..., 0] + 1j * params[..., 1])
    return params                                            # 'com' (and the types JonesResponse finishes)


def complex2params(data, param_type):
    if param_type == 'real':
        return data.real
    if param_type == 'amp':
        return torch.log(torch.abs(data))
    if param_type == 'phs':
        return torch.angle(data)
    if param_type == 'amp_phs':
        return torch.cat([data.abs().log()[..., None], data.angle()[..., None]], dim=-1)
    return data


def rephase_to_refant(params, param_type, refant_idx, p0=None, mode='rephase', inplace=False):
    """
    Reference-antenna phase convention on (Npol, Npol, Nant, Ntimes, Nfreqs[, 2]) parameters (calibration.py:2490-2608):
    'rephase' divides every antenna by the reference antenna's phasor of params + p0 ('com') or subtracts its
    phase / delay ('phs', 'dly', 'amp_phs'); 'zero' only zeroes the reference antenna's imaginary part / phase.
    """
    if refant_idx is None:
        return None
    if p0 is None:
        p0 = torch.zeros_like(params)
    if not inplace:
        params, p0 = copy.deepcopy(params), copy.deepcopy(p0)
    r = slice(refant_idx, refant_idx + 1)
    if mode == 'rephase':
        if param_type == 'com':
            real_view = not torch.is_complex(params)
            _p, _p0 = (utils.viewcomp(params), utils.viewcomp(p0)) if real_view else (params, p0)
            phasor = torch.exp(1j * torch.angle((_p + _p0)[:, :, r]).detach().clone())
            _p, _p0 = _p / phasor, _p0 / phasor
            params[:] = utils.viewreal(_p) if real_view else _p
            p0[:] = utils.viewreal(_p0) if real_view else _p0
        elif param_type in ('dly', 'phs'):
            params -= params[:, :, r].clone()
            p0 -= p0[:, :, r].clone()
        elif param_type == 'amp_phs':
            params[..., 1] -= params[:, :, r, ..., 1].clone()
            p0[..., 1] -= p0[:, :, r, ..., 1].clone()
    elif mode == 'zero':
        for t in (params, p0):
            if param_type == 'com':
                if torch.is_complex(t):
                    t.imag[:, :, r] = torch.zeros_like(t.imag[:, :, r])
                else:
                    t[:, :, r, ..., 1] = torch.zeros_like(t[:, :, r, ..., 1])
            elif param_type in ('dly', 'phs'):
                t[:, :, r] = torch.zeros_like(t[:, :, r])
            elif param_type == 'amp_phs':
                t[:, :, r, ..., 1] = torch.zeros_like(t[:, :, r, ..., 1])
    if not inplace:
        return params, p0


# ---------------------------------------------------------------------------------------
# response functions (calibration.py:11-212, 745-875)
# ---------------------------------------------------------------------------------------
class BaseResponse:
    """params (Npol, Npol, Nant | Nbl, Ntimes | Ncoeff, Nfreqs | Ncoeff) -> complex tensor over (Ntimes, Nfreqs):
    optional LM, complex view, linear bases along frequency / time, + base0, param-type conversion, projection"""
    def __init__(self, freq_mode='channel', time_mode='channel', param_type='com', device=None, freq_LM=None,
                 time_LM=None, freqs=None, times=None, LM=None, projection_kwargs={}, base0=None):
        self.freq_mode, self.time_mode, self.param_type = freq_mode, time_mode, param_type
        self.device = device
        self.freq_LM, self.time_LM, self.LM = freq_LM, time_LM, LM
        self.freqs, self.times = freqs, times
        self.setup_projection(**projection_kwargs)
        self.base0 = base0
        self._args = dict(freq_mode=freq_mode, time_mode=time_mode, param_type=param_type)

    def setup_projection(self, abs_amp_gain=False, phs_slope_gain=False, wgts_gain=None, refant_idx=None):
        """projection of the complex parameters after the response (calibration.py:150-212): abs_amp_gain / phs_slope_gain
        divide the redundant-calibration degeneracies (antenna-averaged amplitude, phase gradient over the array; the latter
        needs self.antpos) out of complex gains, computed with the 1-D antenna weights wgts_gain (default uniform);
        refant_idx rephases to that antenna.  Call it after construction where the subclass sets antpos there."""
        self._proj_abs_amp_gain, self._proj_phs_slope_gain, self._proj_wgts_gain = abs_amp_gain, phs_slope_gain, wgts_gain
        if phs_slope_gain:
            assert getattr(self, 'antpos', None) is not None, 'phs_slope requires antpos'
        self._proj_refant_idx = refant_idx
        self._projection = bool(abs_amp_gain or phs_slope_gain or refant_idx is not None)

    def projection(self, params):
        if not self._projection:
            return params
        if self._proj_abs_amp_gain or self._proj_phs_slope_gain:
            antpos = getattr(self, 'antpos', None)
            ants = None if antpos is None else antpos.ants
            params = remove_redcal_degen(params, ants, antpos, abs_amp=self._proj_abs_amp_gain,
                                         phs_slope=self._proj_phs_slope_gain, wgts=self._proj_wgts_gain)[0]
        if self._proj_refant_idx is not None:
            i = self._proj_refant_idx
            params = params / torch.exp(1j * torch.angle(params[:, :, i:i + 1].detach()))
        return params

    def params2complex(self, params):
        return params2complex(params, self.param_type)

    def forward(self, params, **kwargs):
        if not utils.check_devices(params.device, self.device):
            params = params.to(self.device)
        if self.LM is not None:
            params = self.LM(params)
        if self.param_type == 'com' and not torch.is_complex(params):
            params = utils.viewcomp(params)
        if self.freq_mode == 'linear':
            params = self.freq_LM(params)
        if self.time_mode == 'linear':
            params = self.time_LM(params)
        if self.base0 is not None:
            params = params + self.base0
        params = self.projection(self.params2complex(params))
        if isinstance(params, torch.nn.Parameter):
            params = params.view(params.shape)
        return params

    __call__ = forward

    def push(self, device):
        if not isinstance(device, torch.dtype):
            self.device = device
        if self.base0 is not None:
            self.base0 = utils.push(self.base0, device)
        for lm in (self.LM, self.freq_LM if self.freq_mode == 'linear' else None,
                   self.time_LM if self.time_mode == 'linear' else None):
            if lm is not None and hasattr(lm, 'push'):
                lm.push(device)


class JonesResponse(BaseResponse):
    """gain types 'com', 'real', 'amp', 'phs', 'amp_phs', 'dly' [ns], and the array-gradient types 'dly_slope'
    [ns / m] and 'phs_slope' [rad / m] whose antenna axis holds (EW, NS) (calibration.py:745-875)"""
    def __init__(self, freq_mode='channel', time_mode='channel', param_type='com', vis_type='com', antpos=None,
                 device=None, freq_LM=None, time_LM=None, freqs=None, times=None, LM=None, base0=None):
        super().__init__(freq_mode=freq_mode, time_mode=time_mode, param_type=param_type, device=device,
                         freq_LM=freq_LM, time_LM=time_LM, LM=LM, base0=base0, freqs=freqs, times=times)
        self.vis_type, self.antpos = vis_type, antpos
        assert param_type in ['com', 'amp', 'phs', 'dly', 'real', 'amp_phs', 'phs_slope', 'dly_slope']
        if param_type in ('dly_slope', 'phs_slope'):
            assert antpos is not None, 'need antpos for dly_slope or phs_slope'
            self.antpos_EW = torch.as_tensor([float(antpos[a][0]) for a in antpos], device=device)[None, None, :, None, None]
            self.antpos_NS = torch.as_tensor([float(antpos[a][1]) for a in antpos], device=device)[None, None, :, None, None]
        if 'dly' in param_type:
            assert self.freqs is not None, 'need frequencies for delay gain type'

    def params2complex(self, jones):
        jones = super().params2complex(jones)
        if self.param_type == 'dly' and self.vis_type == 'com':
            return torch.exp(2j * np.pi * jones * torch.as_tensor(self.freqs / 1e9, dtype=jones.dtype, device=jones.device))
        if self.param_type in ('dly_slope', 'phs_slope'):
            tot = jones[:, :, :1] * self.antpos_EW + jones[:, :, 1:] * self.antpos_NS
            if self.param_type == 'phs_slope':
                return torch.exp(1j * tot)
            if self.vis_type == 'com':
                return torch.exp(2j * np.pi * tot * torch.as_tensor(self.freqs, device=tot.device) / 1e9)
            return tot
        return jones

    def push(self, device):
        super().push(device)
        if self.param_type in ('dly_slope', 'phs_slope') and not isinstance(device, torch.dtype):
            self.antpos_EW, self.antpos_NS = self.antpos_EW.to(device), self.antpos_NS.to(device)


class IndexCache:
    """time / baseline index caches for minibatched inputs of shape (..., Nbls, Ntimes, Nfreqs) (calibration.py:291-413)"""
    def __init__(self, times=None, bls=None, atol=1e-5):
        self._times, self._bls, self._atol = times, bls, atol
        self.clear_time_cache()
        self.clear_bl_cache()

    def clear_time_cache(self):
        self.cache_tidx = {}

    def clear_bl_cache(self):
        self.cache_bidx = {}

    def get_time_idx(self, times):
        if times is None or getattr(self, '_times', None) is None:
            return None
        h = utils.arr_hash(times)
        if h not in self.cache_tidx:
            ref = torch.as_tensor(self._times)
            idx = torch.cat([torch.where(torch.isclose(ref, torch.as_tensor(t, dtype=ref.dtype, device=ref.device),
                                                       atol=self._atol, rtol=1e-15))[0] for t in times])
            self.cache_tidx[h] = utils._list2slice(idx)
        return self.cache_tidx[h]

    def get_bl_idx(self, bls):
        if bls is None or getattr(self, '_bls', None) is None:
            return None
        h = utils.arr_hash(bls)
        if h not in self.cache_bidx:
            if isinstance(bls, list):
                idx = [self._bls.index(bl) for bl in bls]
            elif isinstance(bls, torch.Tensor):
                idx = torch.cat([torch.where(self._bls == bl)[0] for bl in bls])
            else:
                idx = np.concatenate([np.where(self._bls == bl)[0] for bl in bls])
            self.cache_bidx[h] = utils._list2slice(idx)
        return self.cache_bidx[h]

    def index_params(self, params, times=None, bls=None):
        for sel, axis in ((self.get_time_idx(times) if times is not None else None, -2),
                          (self.get_bl_idx(bls) if bls is not None else None, -3)):
            if sel is None:
                continue
            if isinstance(sel, slice) and (sel.stop - sel.start) // sel.step == params.shape[axis]:
                continue
            params = params[..., sel, :] if axis == -2 else params[..., sel, :, :]
        return params


class _CalTerm(utils.Module, IndexCache):
    """
    What the calibration terms (JonesModel, RedVisModel / VisModel, VisCoupling, RedVisCoupling) share: the constructor head,
    the caches with the cached output VisData `_vd`, the chain parameters -> response -> hooks -> priors (_response) and push.
    A new term adds its indexing and its `ops` call, not another copy of these.
    """
    _clear_on_push = None            # name of the cache-clearing method that a push to a device calls
    _push_names = ()                 # tensor (or tuple-of-tensor) attributes of the class that push moves, where they exist

    def __init__(self, params, R, parameter=True, p0=None, name=None, atol=1e-5, bls=None):
        utils.Module.__init__(self, name=name)
        self.params = torch.nn.Parameter(params) if parameter else params
        self.p0 = p0
        self.device = params.device
        self.R = R
        IndexCache.__init__(self, times=getattr(self.R, 'times', None), bls=bls, atol=atol)
        self.clear_cache()

    def clear_cache(self):
        """clear all caches, some come from IndexCache"""
        self.clear_time_cache()
        self.clear_bl_cache()
        self.clear_vd_cache()

    def clear_vd_cache(self):
        self._vd = None

    def __getstate__(self):
        """pickle and deepcopy leave the cached output behind: after a forward its data is a node of an autograd graph"""
        state = dict(self.__dict__)
        state['_vd'] = None
        return state

    def _response(self, prior_cache, out=None):
        """params (+ p0) -> R (unless its output `out` is given) -> gradient hooks -> priors into prior_cache"""
        if out is None:
            out = self.R(self._full_params())
        self._hook_response(out)
        self.eval_prior(prior_cache, inp_params=self.params, out_params=out)
        return out

    def push(self, device):
        """push to a new device or dtype"""
        if not isinstance(device, torch.dtype):
            if self._clear_on_push is not None:
                getattr(self, self._clear_on_push)()
            self.device = device
            if isinstance(self._times, torch.Tensor):
                self._times = utils.push(self._times, device)
            if isinstance(self._bls, torch.Tensor):
                self._bls = utils.push(self._bls, device)
        for k in self._push_names:
            v = getattr(self, k, None)
            if v is not None:
                setattr(self, k, tuple(utils.push(a, device) for a in v) if isinstance(v, tuple) else utils.push(v, device))
        self._push_params(device)


class JonesModel(_CalTerm):
    """
    Antenna-based, direction-independent Jones term V^d_pq = J_p V^m_pq J_q^dagger applied to a VisData
    (calibration.py:416-742): 1-pol (1, 1), 2-pol (diagonal) and 4-pol (full 2 x 2) parameters of shape
    (Npol, Npol, Nant, Ntimes | Ncoeff, Nfreqs | Ncoeff); forward(vd, undo=False, prior_cache=None, jones=None) -> VisData.
    """
    _clear_on_push = 'clear_cache'   # a device push drops every cache

    def __init__(self, params, ants, p0=None, refant=None, R=None, parameter=True, polmode='1pol', single_ant=False,
                 name=None, vis_type='com', atol=1e-5):
        super().__init__(params, R if R is not None else JonesResponse(), parameter=parameter, p0=p0, name=name, atol=atol)
        self.ants = list(ants)
        self.Nants = len(self.ants)
        self.polmode, self.single_ant, self.vis_type = polmode, single_ant, vis_type
        self.set_refant(refant)
        self._args = dict(refant=refant, polmode=polmode)
        self._args[self.R.__class__.__name__] = getattr(self.R, '_args', None)

    def clear_cache(self):
        super().clear_cache()
        self.cache_aidx = {}

    def clear_ant_cache(self):
        self.cache_aidx = {}

    def get_ant_idx(self, bls):
        """(g1_idx, g2_idx): antenna-axis indices of the two gains of every baseline, cached by the baseline array"""
        h = utils.arr_hash(bls)
        if h not in self.cache_aidx:
            if self.single_ant:
                i1 = i2 = [0] * len(bls)
            else:
                pairs = utils.blnum2ants(bls)
                where = {a: i for i, a in enumerate(self.ants)}
                i1, i2 = [where[b[0]] for b in pairs], [where[b[1]] for b in pairs]
            self.cache_aidx[h] = (torch.as_tensor(i1, dtype=torch.int32, device=self.device),
                                  torch.as_tensor(i2, dtype=torch.int32, device=self.device))
        return self.cache_aidx[h]

    def set_refant(self, refant):
        self.refant, self.refant_idx, self.rephase_mode = refant, None, None
        if refant is not None:
            assert refant in self.ants, "need a valid refant"
            self.refant_idx = self.ants.index(refant)
            channel = self.R.time_mode == 'channel' and self.R.freq_mode == 'channel'
            self.rephase_mode = 'rephase' if channel else 'zero'
            self.fix_refant_phs()

    def fix_refant_phs(self):
        with torch.no_grad():
            rephase_to_refant(self.params, self.R.param_type, self.refant_idx, p0=self.p0, mode=self.rephase_mode,
                              inplace=True)

    def forward(self, vd, undo=False, prior_cache=None, jones=None):
        if self.refant_idx is not None:
            self.fix_refant_phs()
        if getattr(self, '_vd', None) is None:
            self._vd = vd.copy(copydata=True, copymeta=True)        # a full copy is cached and a fresh copy returned
        vout = self._vd.copy(copydata=False, copymeta=False)
        jones = self.index_params(self._response(prior_cache, out=jones), times=vd.times)
        g1_idx, g2_idx = self.get_ant_idx(vd._blnums)
        vout.data, _ = _apply_cal(vd.data, jones, g1_idx, g2_idx, cal_2pol=self.polmode == '2pol',
                                  vis_type=self.vis_type, undo=undo)
        return vout


# ---------------------------------------------------------------------------------------
# redundant calibration: visibility models (calibration.py:877-1255)
# ---------------------------------------------------------------------------------------
class VisModelResponse(BaseResponse):
    """response of VisModel / RedVisModel: params -> complex (Npol, Npol, Nbls | Nred, Ntimes, Nfreqs); param_type 'com'
    (real view, last axis [real, imag]), 'real', 'amp' or 'amp_phs' (calibration.py:1212-1255)"""
    def __init__(self, freq_mode='channel', time_mode='channel', param_type='real', device=None, freqs=None, times=None,
                 freq_LM=None, time_LM=None, LM=None, base0=None):
        super().__init__(freq_mode=freq_mode, time_mode=time_mode, param_type=param_type, device=device, freq_LM=freq_LM,
                         time_LM=time_LM, LM=LM, base0=base0, freqs=freqs, times=times)

    def forward(self, params, bls=None, times=None, **kwargs):
        return super().forward(params)

    __call__ = forward


def _sel2index(sel, N):
    """an IndexCache selection (None, slice, list, array or tensor) along an axis of N entries as an int64 numpy array"""
    if sel is None:
        return np.arange(N)
    if isinstance(sel, slice):
        return np.arange(N)[sel]
    if torch.is_tensor(sel):
        sel = sel.cpu().numpy()
    return np.asarray(sel, dtype=np.int64).reshape(-1)


class _VisTerm(_CalTerm):
    """what RedVisModel and VisModel share: the response output -> ops.redvis with a cached plan"""
    _clear_on_push = 'clear_cache'   # a device push drops every cache

    def __init__(self, params, R, parameter, p0, name, atol, bls=None):
        super().__init__(params, R if R is not None else VisModelResponse(), parameter=parameter, p0=p0, name=name,
                         atol=atol, bls=bls)

    def clear_time_cache(self):      # the plans hold time and baseline indices: either clear drops them too
        self.cache_tidx, self.cache_plan = {}, {}

    def clear_bl_cache(self):
        self.cache_bidx, self.cache_plan = {}, {}

    def _time_index(self, vd, Ntm):
        """(tmap or None for the identity, cache key): the model time of every time of vd"""
        Nt = vd.data.shape[-2]
        sel = self.get_time_idx(vd.times) if (Ntm != Nt or self._select_equal_times) else None
        if sel is None or (isinstance(sel, slice) and len(range(*sel.indices(Ntm))) == Ntm):
            assert Ntm == Nt, 'model of %d times, input of %d and no time index to select with' % (Ntm, Nt)
            return None, None
        return _sel2index(sel, Ntm), utils.arr_hash(vd.times)

    def _apply(self, vd, model, red, Nred, bkey, undo):
        _require_gpu(vd.data)
        if getattr(self, '_vd', None) is None:
            self._vd = vd.copy(copydata=False)
        vout = self._vd
        if model.shape[-2] == 1 and vd.data.shape[-2] > 1:
            model = model.expand(model.shape[:3] + (vd.data.shape[-2],) + model.shape[4:])     # one model time for all: read in place
        Ntm = model.shape[-2]
        tmap, tkey = self._time_index(vd, Ntm)
        key = (bkey, tkey, Nred, Ntm, vd.data.shape[-3], vd.data.shape[-2])
        if key not in self.cache_plan:
            self.cache_plan[key] = ops.RedVisPlan(red(), Nred, tmap=tmap, Ntm=Ntm)
        if model.shape[-1] == 1 and vd.data.shape[-1] > 1:
            model = model.expand(model.shape[:4] + (vd.data.shape[-1],))
        vout.data = ops.redvis(vd.data, model, self.cache_plan[key], undo=undo)
        return vout


class RedVisModel(_VisTerm):
    """
    Redundant visibility model V^d_jk = V^r + V^m_jk (calibration.py:877-1053): params (Npol, Npol, Nredvis, Ntimes | Ncoeff,
    Nfreqs | Ncoeff[, 2]) hold one visibility per redundant group; bl2red maps a baseline -- an antenna-pair tuple, as
    telescope_model.build_reds returns it, or a baseline number -- to its index along Nredvis.  forward(vd, undo=False,
    prior_cache=None) adds (undo: subtracts) the model of every baseline's group to vd.data on the fused kernel of ops.redvis,
    selecting the times of a minibatch through the time index cache; a model whose baseline axis already equals the input's is
    added baseline by baseline.  Returns the cached output VisData with new data, as the reference does.
    """
    _select_equal_times = True       # the reference indexes the model's time axis whenever the response knows the times

    def __init__(self, params, bl2red, R=None, parameter=True, p0=None, name=None, atol=1e-5):
        super().__init__(params, R, parameter, p0, name, atol)
        self.bl2red = bl2red

    def get_bl_idx(self, bls):
        """index tensor that expands the Nredvis axis to the baselines `bls` (baseline numbers); overloads IndexCache.get_bl_idx"""
        h = utils.arr_hash(bls)
        if h not in self.cache_bidx:
            def look(bl):
                return self.bl2red[bl] if bl in self.bl2red else self.bl2red[utils.blnum2ants(int(bl))]
            nums = bls.cpu().numpy() if isinstance(bls, torch.Tensor) else bls
            self.cache_bidx[h] = torch.as_tensor([look(bl) for bl in nums], device=self.device)
        return self.cache_bidx[h]

    def forward(self, vd, undo=False, prior_cache=None):
        redvis = self._response(prior_cache)
        Nbl, Nred = vd.data.shape[-3], redvis.shape[-3]
        if Nred != Nbl:
            return self._apply(vd, redvis, lambda: self.get_bl_idx(vd._blnums), Nred, utils.arr_hash(vd._blnums), undo)
        return self._apply(vd, redvis, lambda: np.arange(Nbl), Nred, None, undo)


class VisModel(_VisTerm):
    """
    Visibility model V^d_jk = V^v_jk + V^m_jk (calibration.py:1056-1209): params (Npol, Npol, Nbl, Ntimes | Ncoeff,
    Nfreqs | Ncoeff[, 2]) ordered like the input of forward; `blnums` (the baseline numbers along Nbl) is only needed for
    baseline minibatches.  Runs the kernel of RedVisModel with the baseline selection in place of the group map.
    """
    _select_equal_times = False      # ... and here only when the input holds fewer times than the model

    def __init__(self, params, R=None, parameter=True, p0=None, blnums=None, name=None, atol=1e-5):
        super().__init__(params, R, parameter, p0, name, atol, bls=blnums)

    def forward(self, vd, undo=False, prior_cache=None, **kwargs):
        vis = self._response(prior_cache)
        Nbl, Nmod = vd.data.shape[-3], vis.shape[-3]
        if Nmod != Nbl:
            assert self._bls is not None, 'a baseline minibatch needs blnums'
            return self._apply(vd, vis, lambda: _sel2index(self.get_bl_idx(vd._blnums), Nmod), Nmod,
                               utils.arr_hash(vd._blnums), undo)
        return self._apply(vd, vis, lambda: np.arange(Nbl), Nmod, None, undo)


# ---------------------------------------------------------------------------------------
# antenna mutual coupling (calibration.py:1258-1586)
# ---------------------------------------------------------------------------------------
def _coupling_delay(lengths, freqs, min_dly, sign, c):
    """complex128 numpy phasor exp(sign 2 pi i (f - f_0) / c * max(min_dly, length)), shape lengths.shape + (Nfreqs,)"""
    if min_dly is not None:
        lengths = np.maximum(lengths, min_dly)
    fr = np.asarray(torch.as_tensor(freqs).detach().cpu(), dtype=np.float64)
    return np.exp(1j * (2 * np.pi * sign * (fr - fr[0]) / c * lengths[..., None]))


def _check_bls(bls, known, who):
    """ValueError for the first baseline that names an antenna outside `known`, has ant2 < ant1 or appeared before (tested in
    that order); `who` is the class named in the message"""
    seen = set()
    for bl in bls:
        bl = tuple(bl)
        if bl[0] not in known or bl[1] not in known:
            raise ValueError('baseline %s names an antenna that is not in antpos' % (bl,))
        if bl[1] < bl[0]:
            raise ValueError('baseline %s: %s needs ant2 >= ant1' % (bl, who))
        if bl in seen:
            raise ValueError('baseline %s appears twice' % (bl,))
        seen.add(bl)


class _CouplingTerm(_CalTerm):
    """what VisCoupling and RedVisCoupling add to _CalTerm: the array attributes, the guards of a forward that needs
    setup_coupling(), and a coupling of one time bin that broadcasts"""
    def __init__(self, params, freqs, antpos, R, parameter, p0, name, atol):
        super().__init__(params, R if R is not None else VisModelResponse(), parameter=parameter, p0=p0, name=name, atol=atol)
        self.freqs = freqs
        self.Nfreqs = len(freqs)
        self.antpos = antpos
        self.Nants = len(antpos)
        self.c = 2.99792458e8
        self.Npol = params.shape[0]
        assert self.Npol == 1, "multi-pol not currently supported"

    def index_params(self, params, times=None):
        """overloads IndexCache.index_params: one time bin in params broadcasts"""
        if times is not None and params.shape[-2] != 1:
            params = IndexCache.index_params(self, params, times=times)
        return params

    def _check_input(self, vd, Nbl_attr):
        """the guards of forward: setup_coupling() has run, GPU tensors, the baselines the plan was set up for"""
        who = type(self).__name__
        if getattr(self, 'plan', None) is None:
            raise RuntimeError('%s: run setup_coupling() before forward()' % who)
        _require_gpu(vd.data)
        Nbl = getattr(self.plan, Nbl_attr)
        if tuple(vd.data.shape[:3]) != (1, 1, Nbl):
            raise ValueError('input of shape %s, %s was set up for (1, 1, %d, Ntimes, Nfreqs)' % (tuple(vd.data.shape), who, Nbl))

    def _coupling(self, vd, prior_cache):
        """the response output at the times of vd, complex in the precision of the data"""
        coupling = self.index_params(self._response(prior_cache), times=vd.times)
        return coupling if coupling.is_complex() else coupling.to(vd.data.dtype)


class VisCoupling(_CouplingTerm):
    """
    Mutual coupling of antennas as a linear map of visibilities across the baseline axis (calibration.py:1258-1586): with V
    the Nant x Nant matrix of all visibilities of one time and channel (lower triangle the conjugate of the upper, baselines
    missing from the input zero) the coupled visibilities are Vc = E V E^H with E = I + X o D, X the coupling coefficients
    (params through the response R, shape (1, 1, Nant, Nant, Ntimes | 1, Nfreqs | 1)) and D the delay phasor between the two
    antennas; `double` adds the double-path term, E = I + Xd + Xd Xd with Xd = X o D.  The matrix order is the order of
    `antpos`; `bls` are the baselines along the Nbls axis of the input, each with ant2 >= ant1.  setup_coupling() must run
    before forward().  forward(vd, prior_cache=None, add_I=None, prod=None, double=False) -> VisData: everything runs in
    ops.coupling_apply -- the matrix is read from vd.data through an index table and only the rows of `bls` are written, so no
    (Nant^2, Ntimes, Nfreqs) copy exists, E is built on the fly and the output of R is never modified in place; the gradients
    come from the same kernel in a fixed summation order (bit-identical from run to run).  As in the reference the `double`
    keyword of forward decides, self.double only when None is passed.  Single polarisation only; no CPU implementation.
    The form fitted on a redundant array, with one coefficient per coupling vector (gen_coupling_terms), is RedVisCoupling;
    CouplingInflate turns its parameters into the matrix used here.  Not built: CouplingExpand.
    """
    # a device push clears no cache here (_clear_on_push stays None)
    _push_names = ('flat_data_idx', 'flat_data_null', 'flat_conj_idx', 'flat_unconj_idx', 'bls_idx', 'I', 'dly', 'freqs')

    def __init__(self, params, freqs, antpos, bls, R=None, parameter=True, p0=None, name=None, atol=1e-5, add_I=True,
                 prod='both', double=False):
        super().__init__(params, freqs, antpos, R, parameter, p0, name, atol)
        self.bls = bls
        self.add_I, self.prod, self.double = add_I, prod, double

    def setup_coupling(self, bls=None, min_dly=None, conj=True):
        """
        Delay phasor and matrix indexing of the forward model.  bls: the baselines of the input data (default: those given
        at construction); min_dly: shortest baseline length [m] used for the coupling delay, dly = max(min_dly, |r_j - r_i|) / c
        (typically the feed height); conj: the conjugated convention of the delay term.  Sets `dly`
        (1, 1, Nant, Nant, 1, Nfreqs) = exp(+-2 pi i (f - f_0) / c * length), the int32 matrix table of ops.CouplingPlan, and
        the reference's index attributes flat_data_idx, flat_conj_idx, flat_unconj_idx, flat_data_null, bls_idx and I.
        ValueError for a baseline with ant2 < ant1, a duplicate or an antenna that is not in antpos (the reference indexes
        the wrong rows without a word).
        """
        if bls is not None:
            self.bls = bls
        ants = [int(a) for a in self.antpos]
        where = {a: i for i, a in enumerate(ants)}
        N = self.Nants
        pairs = [(int(b[0]), int(b[1])) for b in self.bls]
        _check_bls(pairs, where, 'VisCoupling')
        rows = {bl: r for r, bl in enumerate(pairs)}

        # delay phasor between coupled antennas
        vecs = np.stack([np.asarray(torch.as_tensor(self.antpos[a]).detach().cpu(), dtype=np.float64) for a in ants])
        dly = _coupling_delay(np.linalg.norm(vecs[None, :, :] - vecs[:, None, :], axis=-1), self.freqs, min_dly,
                              1 if conj else -1, self.c)
        self.dly = torch.as_tensor(dly[None, None, :, :, None, :]).to(dtype=utils._cfloat(), device=self.device)

        # matrix entry (i, j): the row of (ant_i, ant_j) when ant_j >= ant_i, else the conjugate of the row of (ant_j, ant_i)
        table = np.full((N, N), -1, dtype=np.int64)
        data_idx, null, conj_idx, unconj_idx = [], [], [], []
        for i, a1 in enumerate(ants):
            for j, a2 in enumerate(ants):
                upper = a2 >= a1
                r = rows.get((a1, a2) if upper else (a2, a1))
                (unconj_idx if upper else conj_idx).append(i * N + j)
                data_idx.append(0 if r is None else r)
                null.append(r is None)
                if r is not None:
                    table[i, j] = r if upper else r | ops.COUPLING_CONJ
        out_rows = np.array([where[a1] * N + where[a2] for a1, a2 in pairs], dtype=np.int64)
        self.plan = ops.CouplingPlan(table, out_rows, len(pairs))
        self.flat_data_idx = torch.tensor(data_idx, dtype=torch.int64, device=self.device)
        self.flat_conj_idx = torch.tensor(conj_idx, dtype=torch.int64, device=self.device)
        self.flat_unconj_idx = torch.tensor(unconj_idx, dtype=torch.int64, device=self.device)
        self.flat_data_null = torch.tensor(null, dtype=torch.bool, device=self.device)
        self.bls_idx = torch.as_tensor(out_rows, device=self.device)
        self.I = torch.eye(N, dtype=utils._float(), device=self.device)[None, None, :, :, None, None]

    def forward(self, vd, prior_cache=None, add_I=None, prod=None, double=False, **kwargs):
        """vd: VisData of shape (1, 1, Nbls, Ntimes, Nfreqs) holding exactly the baselines of setup_coupling, in their order;
        returns the cached output VisData with the coupled visibilities"""
        self._check_input(vd, 'Nbl')
        if getattr(self, '_vd', None) is None:
            self._vd = vd.copy(copydata=False)
        vout = self._vd
        coupling = self._coupling(vd, prior_cache)
        double = double if double is not None else self.double
        out = ops.coupling_apply(coupling[0, 0], self.dly[0, 0], vd.data[0, 0], self.plan,
                                 add_I=add_I if add_I is not None else self.add_I,
                                 prod=prod if prod is not None else self.prod, double=bool(double))
        vout.data = out[None, None]
        return vout


# ---------------------------------------------------------------------------------------
# mutual coupling of a redundant model (calibration.py:1588-2175, 3047-3400)
# ---------------------------------------------------------------------------------------
def _antvecs(antpos):
    """(antenna keys, (Nant, 3) numpy positions in the dtype antpos holds) in the order of antpos"""
    ants = list(antpos.keys())
    return ants, np.stack([np.asarray(torch.as_tensor(antpos[a]).detach().cpu()) for a in ants])


def _cut_matrix(vecs, min_len=None, max_len=None, min_EW=None, max_EW=None, min_NS=None, max_NS=None):
    """cut_bl for every ordered antenna pair at once: cut[p, q] for the vector r_q - r_p"""
    d = vecs[None, :, :] - vecs[:, None, :]
    length, ew = np.linalg.norm(d, axis=-1), np.abs(d[..., 0])
    cut = np.zeros(length.shape, dtype=bool)
    if min_len is not None:
        cut |= length < min_len
    if max_len is not None:
        cut |= length > max_len
    if min_EW is not None:
        cut |= ew < min_EW
    if max_EW is not None:
        cut |= ew > max_EW
    if min_NS is not None:                               # the reference tests the East-West component here too (:3395-3398)
        cut |= ew < min_NS
    if max_NS is not None:
        cut |= ew > max_NS
    return cut


def cut_bl(bl, antpos, bl_vecs=None, min_len=None, max_len=None, min_EW=None, max_EW=None, min_NS=None, max_NS=None):
    """
    True if the antenna pair `bl` is cut by its vector r_bl[1] - r_bl[0] (calibration.py:3342-3400): shorter than min_len,
    longer than max_len, East-West extent below min_EW or above max_EW.  As in the reference the North-South limits are
    compared with the East-West component as well.  bl_vecs: optional cache {bl: (vector, length)}.
    """
    if all(x is None for x in (min_len, max_len, min_EW, max_EW, min_NS, max_NS)):
        return False
    if bl_vecs is not None and bl in bl_vecs:
        vec, vec_len = bl_vecs[bl]
    else:
        vec = antpos[bl[1]] - antpos[bl[0]]
        vec_len = torch.linalg.norm(vec)
        if bl_vecs is not None:
            bl_vecs[bl] = vec, vec_len
    ew = abs(vec[0])
    return bool((min_len is not None and vec_len < min_len) or (max_len is not None and vec_len > max_len)
                or (min_EW is not None and ew < min_EW) or (max_EW is not None and ew > max_EW)
                or (min_NS is not None and ew < min_NS) or (max_NS is not None and ew > max_NS))


def gen_coupling_terms(antpos, min_len=None, max_len=None, max_EW=None, max_NS=None, ants=None, no_auto_coupling=False,
                       compress_to_red=False, redtol=1.0):
    """
    Coupling terms (ant_i, ant_j) to model and the index of every term along the Ncoupling axis of the parameters
    (calibration.py:3246-3339): all ordered pairs of antpos whose vector r_j - r_i passes the cuts (length, |East-West|,
    |North-South|), with ant_j in `ants` when given, without the autos under no_auto_coupling.  compress_to_red: one term
    per unique vector within redtol (a pair and its reverse are different vectors); coupling_idx then maps every pair to the
    term of its vector.  Returns (coupling_terms, coupling_idx).
    """
    assert isinstance(antpos, dict) or hasattr(antpos, 'keys')
    keys, vecs = _antvecs(antpos)
    d = vecs[None, :, :] - vecs[:, None, :]                          # d[i, j] = r_j - r_i
    length = np.linalg.norm(d, axis=-1)
    keep = np.ones(length.shape, dtype=bool)
    if no_auto_coupling:
        keep &= ~np.eye(len(keys), dtype=bool)
    if ants is not None:
        keep &= np.array([k in ants for k in keys], dtype=bool)[None, :]
    if min_len is not None:
        keep &= ~(length < min_len)
    if max_len is not None:
        keep &= ~(length > max_len)
    if max_EW is not None:
        keep &= ~(np.abs(d[..., 0]) > max_EW)
    if max_NS is not None:
        keep &= ~(np.abs(d[..., 1]) > max_NS)
    ii, jj = np.nonzero(keep)                                        # row-major: the reference's loop order
    coupling_terms = [(keys[i], keys[j]) for i, j in zip(ii, jj)]
    coupling_idx = {c: i for i, c in enumerate(coupling_terms)}
    if compress_to_red:
        cvec = d[ii, jj]
        red_vecs, first, red_idx = np.zeros((0, 3), dtype=cvec.dtype), [], []
        for n, v in enumerate(cvec):                                 # first group within redtol, else a new one
            match = np.nonzero(np.linalg.norm(red_vecs - v, axis=1) < redtol)[0]
            if match.size:
                red_idx.append(int(match[0]))
            else:
                red_idx.append(len(first))
                red_vecs = np.concatenate([red_vecs, v[None]])
                first.append(n)
        coupling_idx = {c: red_idx[i] for i, c in enumerate(coupling_terms)}
        coupling_terms = [coupling_terms[n] for n in first]
    return coupling_terms, coupling_idx


def configure_coupling_matrix_singlepath(antpos, bls, bl2red=None, no_auto_coupling=False, include_second_order=True,
                                         min_len=None, max_len=None, max_EW=None, max_NS=None, second_max_len=None,
                                         second_max_EW=None, second_max_NS=None, Nproc=None, Ntask=5, use_pathos=True):
    """
    Rows of the baseline-to-baseline matrix of single-path mutual coupling, Vc = E V E^H with E = I + X
    (calibration.py:3052-3243).  For the output baseline (j, k) antenna i contributes the first-order terms eps_j_i V_ik and
    conj(eps_k_i) V_ji and, with include_second_order, eps_j_i conj(eps_k_i') V_ii' for every i'.  Returns
    Arows: {output baseline: {input baseline: ['eps_j_i', 'eps_k_i_conj', 'eps_j_i,eps_k_i2_conj', ...]}} with the
    reference's keys, names and list order.  bl2red: physical baseline (both orientations) -> the redundant baseline that
    stands for it; a visibility that it does not hold is dropped.  A term whose vector is cut (min_len, max_len, max_EW,
    max_NS for the first order; min_len and second_max_* for both factors of the second) is left out, and so are the auto
    terms under no_auto_coupling (of a second-order product only its conjugated factor is tested, as in the reference).
    The cuts are evaluated for all antenna pairs at once with numpy; Nproc, Ntask and use_pathos are accepted and ignored.
    """
    keys, vecs = _antvecs(antpos)
    where = {a: i for i, a in enumerate(keys)}
    N = len(keys)
    keep1 = ~_cut_matrix(vecs, min_len=min_len, max_len=max_len, max_EW=max_EW, max_NS=max_NS)
    keep2 = ~_cut_matrix(vecs, min_len=min_len, max_len=second_max_len, max_EW=second_max_EW, max_NS=second_max_NS)
    auto = np.eye(N, dtype=bool)
    if no_auto_coupling:
        keep1 &= ~auto
    look = (lambda bl: bl2red.get(bl)) if bl2red else (lambda bl: bl)
    Arows = {}
    for bl in bls:
        p0, p1 = where[bl[0]], where[bl[1]]
        first0, first1 = keep1[p0], keep1[p1]
        row = {}
        if include_second_order:
            sec0 = keep2[p0]
            sec1 = np.nonzero(keep2[p1] & ~auto[p1] if no_auto_coupling else keep2[p1])[0]
        for k in range(N):
            ant = keys[k]
            if first0[k]:
                vis = look((ant, bl[1]))
                if vis is not None:
                    row.setdefault(vis, []).append('eps_{}_{}'.format(bl[0], ant))
            if first1[k]:
                vis = look((bl[0], ant))
                if vis is not None:
                    row.setdefault(vis, []).append('eps_{}_{}_conj'.format(bl[1], ant))
            if include_second_order and sec0[k]:
                for k2 in sec1:
                    vis = look((ant, keys[k2]))
                    if vis is not None:
                        row.setdefault(vis, []).append('eps_{}_{},eps_{}_{}_conj'.format(bl[0], ant, bl[1], keys[k2]))
        Arows[bl] = row
    return Arows


class CouplingInflate:
    """
    Inflates the parameters of a RedVisCoupling (one per coupling vector) to the Nants x Nants coupling matrix of a
    VisCoupling, in the order of antpos (calibration.py:2118-2175): entry (i, j) takes the term whose vector matches
    r_i - r_j within redtol, zero where none does.  vecs (Nterms, 3) ENU [m].  __call__(params (Npol, Npol, Nterms, Ntimes,
    Nfreqs)) -> (Npol, Npol, Nants, Nants, Ntimes, Nfreqs) by one gather and a fill, without writing into its input.
    """
    def __init__(self, vecs, antpos, redtol=1.0):
        self.vecs, self.antpos, self.redtol = vecs, antpos, redtol
        self.ants, pos = _antvecs(antpos)
        Nants = len(self.ants)
        self.shape = (Nants, Nants)
        v = np.asarray(torch.as_tensor(vecs).detach().cpu())
        d = pos[:, None, :] - pos[None, :, :]                         # d[i, j] = r_i - r_j
        match = np.linalg.norm(v[None, None, :, :] - d[:, :, None, :], axis=-1) <= redtol
        self.idx = torch.as_tensor(np.where(match.any(axis=-1), match.argmax(axis=-1), 0).ravel(), dtype=torch.int64)
        self.zeros = torch.as_tensor(~match.any(axis=-1).ravel())

    def __call__(self, params):
        shape = params.shape[:2] + self.shape + params.shape[-2:]
        out = params.index_select(2, self.idx.to(params.device))
        return out.masked_fill(self.zeros.to(params.device)[None, None, :, None, None], 0.0).reshape(shape)

    def push(self, device):
        self.idx = utils.push(self.idx, device)
        self.zeros = utils.push(self.zeros, device)


_RVC_TUPLES = ('unconj_param_unconj_vis', 'unconj_param_conj_vis', 'conj_param_unconj_vis', 'conj_param_conj_vis',
               'sq_param_unconj_vis', 'sq_param_conj_vis')


class RedVisCoupling(_CouplingTerm):
    """
    Mutual coupling with a redundant visibility model as input and all physical baselines as output
    (calibration.py:1588-2115):  Vc = A @ Vr + B @ conj(Vr),  A and B (Nbls_out, Nbls_in) matrices of the first-order terms
    eps, conj(eps) and the second-order single-path terms eps conj(eps'), eps = R(params) o dly.  params has shape (1, 1,
    Ncoupling, Ntimes | 1, Nfreqs | 1[, 2]) with one row per entry of coupling_terms ((i, j): eps_i_j, v_i <- v_i + eps_i_j v_j);
    coupling_idx maps antenna pairs to rows (pass the one of gen_coupling_terms(..., compress_to_red=True) for one term per
    unique vector).  bls_in: the baselines of the input (with use_reds the redundant baselines), bls_out those of the output,
    each with ant2 >= ant1.  setup_coupling() must run before forward().

    Where the reference fills two dense (Nbls_out, Nbls_in, Ntimes, Nfreqs) matrices and contracts them with einsum, forward
    runs ops.redcoupling_apply on a flat list of the non-zero terms (ops.RedCouplingPlan): the zeroth-order term -- with
    use_reds the inflation by redundancy -- is one more entry per output row, no matrix and no inflated copy exists, and the
    gradients are summed in an order fixed by the plan (bit-identical from run to run).  The reference's indexed `+=` keeps
    one of two terms of one kind that fall on the same matrix element; here they add.  With neither kind of first-order
    term on a visibility (plain / conjugated) the reference skips its second-order terms too, and so does the plan.
    Single polarisation; no CPU implementation.
    """
    _clear_on_push = 'clear_vd_cache'          # a device push drops only the cached output
    _push_names = _RVC_TUPLES + ('dly',)

    def __init__(self, params, freqs, antpos, coupling_terms, bls_in, bls_out, coupling_idx=None, R=None, parameter=True,
                 p0=None, name=None, atol=1e-5):
        super().__init__(params, freqs, antpos, R, parameter, p0, name, atol)
        self.coupling_terms = coupling_terms
        self.coupling_idx = coupling_idx if coupling_idx is not None else {c: i for i, c in enumerate(coupling_terms)}
        self.Nterms = len(coupling_terms)
        self.bls_in, self.bls_out = bls_in, bls_out
        self.plan = None

    def setup_coupling(self, use_reds=True, copydata=False, redtol=1.0, include_second_order=True, min_len=None,
                       max_len=None, max_EW=None, max_NS=None, second_max_len=None, second_max_EW=None, second_max_NS=None,
                       min_dly=None, Nproc=None, Ntask=5, use_pathos=True):
        """
        Delay phasor and indexing of the forward model.  use_reds: bls_in are redundant baselines (else the physical ones,
        bls_in == bls_out); copydata: kept for the reference's signature, the input is never modified; redtol [m] for the
        redundancy; include_second_order, min_len, max_len, max_EW, max_NS, second_max_*: the terms to include, see
        configure_coupling_matrix_singlepath; min_dly: shortest length [m] used for the coupling delay.  Sets `dly`
        (1, 1, Nterms, 1, Nfreqs) = exp(2 pi i (f - f_0) / c * max(min_dly, |r_j - r_i|)), the reference's index tuples
        unconj_param_unconj_vis, unconj_param_conj_vis, conj_param_unconj_vis, conj_param_conj_vis ((rows, columns, terms))
        and sq_param_unconj_vis, sq_param_conj_vis ((rows, columns, element of every product, first and conjugated term)),
        with use_reds `red_bl_inds`, and `plan`, the ops.RedCouplingPlan of all of them.  ValueError for an output baseline
        with ant2 < ant1, a duplicate, or an antenna that is not in antpos.  Nproc, Ntask, use_pathos: ignored.
        """
        known = set(self.antpos.keys())
        _check_bls(self.bls_out, known, 'RedVisCoupling')
        for ct in self.coupling_terms:
            if ct[0] not in known or ct[1] not in known:
                raise ValueError('coupling term %s names an antenna that is not in antpos' % (tuple(ct),))
        self.use_reds, self.copydata = use_reds, copydata
        bl2red = None
        if use_reds:
            reds, _, bl2red_idx, _, _, _, _ = telescope_model.build_reds(self.antpos, bls=self.bls_out, red_bls=self.bls_in,
                                                                        redtol=redtol)
            bl2red = {}
            for k in bl2red_idx:
                bl2red[k] = reds[bl2red_idx[k]][0]
                bl2red[k[::-1]] = reds[bl2red_idx[k]][0][::-1]

        # delay phasor between coupled antennas
        keys, vecs = _antvecs(self.antpos)
        where = {a: i for i, a in enumerate(keys)}
        vecs = vecs.astype(np.float64)
        length = np.array([np.linalg.norm(vecs[where[a2]] - vecs[where[a1]]) for a1, a2 in self.coupling_terms])
        dly = _coupling_delay(length, self.freqs, min_dly, 1, self.c)
        self.dly = torch.as_tensor(dly[None, None, :, None, :]).to(dtype=utils._cfloat(), device=self.device)

        Arows = configure_coupling_matrix_singlepath(self.antpos, bls=self.bls_out, bl2red=bl2red,
                                                     include_second_order=include_second_order, min_len=min_len,
                                                     max_len=max_len, max_EW=max_EW, max_NS=max_NS,
                                                     second_max_len=second_max_len, second_max_EW=second_max_EW,
                                                     second_max_NS=second_max_NS)
        if use_reds:
            for bl in self.bls_out:
                if bl not in bl2red_idx:
                    raise ValueError('output baseline %s is redundant with none of bls_in' % (tuple(bl),))
            self.red_bl_inds = [bl2red_idx[bl] for bl in self.bls_out]
        elif len(self.bls_in) != len(self.bls_out):
            raise ValueError('without use_reds the input baselines are the output baselines')

        # the index lists of the reference (:1788-1928), visiting only the columns a row names
        first = {k: ([], [], []) for k in _RVC_TUPLES[:4]}
        sq = {0: ([], [], [], [], []), 1: ([], [], [], [], [])}
        counter = [0, 0]
        cols = {}
        for j, bli in enumerate(self.bls_in):
            cols.setdefault(tuple(bli), []).append(j)
        cidx = self.coupling_idx

        def pair(name):
            return tuple(int(a) for a in name.split('_')[1:3])

        for i, blo in enumerate(self.bls_out):
            Arow = Arows[blo]
            js = set()
            for key in Arow:
                js.update(cols.get(key, ()))
                js.update(cols.get(key[::-1], ()))
            for j in sorted(js):
                bli = tuple(self.bls_in[j])
                for cv, key in ((0, bli), (1, bli[::-1])):
                    if key not in Arow or (cv == 1 and bli[0] == bli[1]):
                        continue
                    appended = False
                    for eps in Arow[key]:
                        if ',' in eps:
                            t1, t2 = eps.split(',')
                            c1, c2 = pair(t1), pair(t2)
                            if c1 not in cidx or c2 not in cidx:
                                continue
                            if not appended:
                                sq[cv][0].append(i)
                                sq[cv][1].append(j)
                            sq[cv][2].append(counter[cv])
                            sq[cv][3].append(cidx[c1])
                            sq[cv][4].append(cidx[c2])
                            appended = True
                        else:
                            c = pair(eps)
                            if c not in cidx:
                                continue
                            lst = first[('conj_param_' if 'conj' in eps else 'unconj_param_') + ('conj_vis' if cv else 'unconj_vis')]
                            lst[0].append(i)
                            lst[1].append(j)
                            lst[2].append(cidx[c])
                    counter[cv] += appended
        for k in _RVC_TUPLES[:4]:
            setattr(self, k, tuple(torch.as_tensor(x, dtype=torch.int64) for x in first[k]))
        self.sq_param_unconj_vis = tuple(torch.as_tensor(x, dtype=torch.int64) for x in sq[0])
        self.sq_param_conj_vis = tuple(torch.as_tensor(x, dtype=torch.int64) for x in sq[1])
        self.plan = self._build_plan()
        self.clear_vd_cache()

    def _build_plan(self):
        """every term forward adds up, as one entry list: zeroth order, then per kind of visibility the first-order terms
        and the second-order products (only where the reference builds that matrix at all)"""
        Nout, Nin = len(self.bls_out), len(self.bls_in)
        zero = np.asarray(self.red_bl_inds if self.use_reds else np.arange(Nout), dtype=np.int64)
        row, col, cj = [np.arange(Nout)], [zero], [np.zeros(Nout, dtype=np.int64)]
        a, b = [np.full(Nout, -1)], [np.full(Nout, -1)]
        for cv, (un, co, sq) in enumerate((('unconj_param_unconj_vis', 'conj_param_unconj_vis', 'sq_param_unconj_vis'),
                                           ('unconj_param_conj_vis', 'conj_param_conj_vis', 'sq_param_conj_vis'))):
            un, co, sq = (tuple(np.asarray(x.cpu(), dtype=np.int64) for x in getattr(self, k)) for k in (un, co, sq))
            if len(un[0]) == 0 and len(co[0]) == 0:
                continue
            none = np.full(len(un[0]), -1), np.full(len(co[0]), -1)
            row += [un[0], co[0], sq[0][sq[2]]]
            col += [un[1], co[1], sq[1][sq[2]]]
            a += [un[2], none[1], sq[3]]
            b += [none[0], co[2], sq[4]]
            cj += [np.full(len(un[0]) + len(co[0]) + len(sq[2]), cv, dtype=np.int64)]
        cat = lambda x: np.concatenate([np.asarray(y, dtype=np.int64) for y in x])
        return ops.RedCouplingPlan(cat(row), cat(col), cat(cj), cat(a), cat(b), Nout, Nin, self.Nterms)

    def forward(self, vd, prior_cache=None, **kwargs):
        """vd: VisData of shape (1, 1, Nbls_in, Ntimes, Nfreqs) holding bls_in in their order; returns a VisData of the
        baselines bls_out with the coupled visibilities (cached between calls, with new data)"""
        self._check_input(vd, 'Nin')
        if getattr(self, '_vd', None) is None:
            if self.use_reds:
                take = lambda x: None if x is None else x.index_select(2, torch.as_tensor(self.red_bl_inds, device=x.device))
                by_bl = vd.cov_axis in (None, 'bl')
                self._vd = dataset.VisData()
                self._vd.setup_meta(telescope=vd.telescope, antpos=vd.antpos)
                self._vd.setup_data(self.bls_out, vd.times, vd.freqs, pol=vd.pol, data=None, flags=take(vd.flags),
                                    cov=take(vd.cov) if by_bl else vd.cov, cov_axis=vd.cov_axis,
                                    icov=take(vd.icov) if by_bl else vd.icov, history=vd.history)
            else:
                self._vd = vd.copy(copydata=False)
        vout = self._vd
        coupling = self._coupling(vd, prior_cache)
        out = ops.redcoupling_apply(coupling[0, 0], self.dly[0, 0, :, 0], vd.data[0, 0], self.plan)
        vout.data = out[None, None]
        return vout

    def get_coupling_hits(self):
        """{coupling term: how often the index tuples name its row}, counted as the reference counts (calibration.py:2092-2115:
        the second list of every first-order tuple and the second and third of the second-order ones)"""
        lists = [np.asarray(getattr(self, k)[1].cpu()) for k in _RVC_TUPLES] + \
                [np.asarray(getattr(self, k)[2].cpu()) for k in _RVC_TUPLES[4:]]
        return {ct: int(sum((x == i).sum() for x in lists)) for i, ct in enumerate(self.coupling_terms)}


# ---------------------------------------------------------------------------------------
# partly redundant arrays: sparse learnable mixing of redundant models onto the physical baselines (calibration.py:2178-2344)
# ---------------------------------------------------------------------------------------
def _identity(x):
    """the default response of PartialRedVisInflate (a module-level function, so that the module pickles)"""
    return x


class PartialRedVisInflate(_CalTerm):
    """
    Inflation of a redundant visibility model onto the physical baselines of an array that is only partly redundant
    (calibration.py:2178-2344): out[p, q, i, t, f] = sum_e c_e V[p, q, col_e, t, f] over the non-zero entries e of row i of a
    sparse mixing matrix A of shape `Ashape`, c = R(params + p0) real with one learnable number per entry.  bl2red maps every
    baseline of new_bls to the indices along the Nbls axis of the input that sum to it (a list, or one Python / numpy integer).
    The entries are listed in the order of new_bls and, within a baseline, of bl2red[bl]: `idx` (2, Nnz) holds their (row,
    column), `Nred` the length of the list each belongs to, and params[k] belongs to entry idx[:, k], as the reference's
    docstring and its dense path have it.  (The reference's CSR path sorts the columns of each row and so assigns the
    parameters of an unsorted list to other entries; that is not reproduced.)  The default params, 1 / Nred, average the
    contributing models; a baseline with an empty list gives a zero row.  `use_csr` is accepted for signature compatibility and
    changes nothing: there is one path, ops.partred_inflate -- one pass forward, and both gradients by reductions in an order
    the plan fixes (bit-identical from run to run), where the reference builds a CSR matrix on every forward, copies the data
    with the baseline axis in front and calls torch.sparse.mm twice.
    KeyError for a baseline missing from bl2red; ValueError for a negative column, the same column twice in one baseline, no
    entry at all, params of another length than Nnz and, in forward, input whose baseline axis is not Ashape[1] long.
    forward(vd, prior_cache=None) -> a new VisData of new_bls.  No CPU implementation.
    """
    _clear_on_push = None
    _push_names = ('idx', 'Nred')

    def __init__(self, bl2red, new_bls, params=None, p0=None, R=None, parameter=True, use_csr=True):
        rows, cols, Nred = [], [], []
        for i, bl in enumerate(new_bls):
            red = bl2red[bl]
            red = [int(red)] if isinstance(red, (int, np.integer)) else [int(r) for r in red]
            if any(r < 0 for r in red):
                raise ValueError('baseline %s: negative index %d' % (bl, min(red)))
            if len(set(red)) != len(red):
                raise ValueError('baseline %s names the same redundant visibility twice' % (bl,))
            rows += [i] * len(red)
            cols += red
            Nred += [len(red)] * len(red)
        if not rows:
            raise ValueError('bl2red gives no entry for any baseline of new_bls')
        idx = torch.as_tensor([rows, cols], dtype=torch.int64)
        Nred = torch.as_tensor(Nred, dtype=torch.int64)
        if params is None:
            params = torch.ones(len(rows)) / Nred
        if params.ndim != 1 or params.shape[0] != len(rows):
            raise ValueError('params of shape %s, the mixing matrix has %d entries' % (tuple(params.shape), len(rows)))
        super().__init__(params, R if R is not None else _identity, parameter=parameter, p0=p0)
        self.idx, self.Nred = idx, Nred
        self.Ashape = (len(new_bls), int(max(cols)) + 1)
        self.new_bls = new_bls
        self.use_csr = use_csr
        self.device = None
        self.plan = ops.PartRedPlan(rows, cols, *self.Ashape)

    def _push_params(self, device):
        """overloads utils.Module._push_params: R may be a plain callable without push"""
        self.params = utils.push(self.params, device)
        if hasattr(self.R, 'push'):
            self.R.push(device)
        self.p0 = utils.push(self.p0, device)
        for prs in (self.priors_inp_params, self.priors_out_params):
            for pr in (prs or []):
                if pr is not None:
                    pr.push(device)

    def push(self, device):
        """push params, p0 and the index tensors to a device (the plan's tables follow on their next use), or cast params and
        p0 to a dtype"""
        super().push(device)
        if not isinstance(device, torch.dtype):
            self.plan.tables(device)

    def forward(self, vd, prior_cache=None, **kwargs):
        """vd: VisData of shape (Npol, Npol, Ashape[1], Ntimes, Nfreqs); returns a new VisData of the baselines new_bls"""
        if vd.data.shape[2] != self.Ashape[1]:
            raise ValueError('input of %d baselines, the mixing matrix has %d columns' % (vd.data.shape[2], self.Ashape[1]))
        _require_gpu(vd.data)
        c = self._response(prior_cache)
        real = torch.float32 if vd.data.dtype == torch.complex64 else torch.float64
        data = ops.partred_inflate(vd.data, c.to(real), self.plan)
        new_vis = dataset.VisData()
        new_vis.setup_meta(telescope=vd.telescope, antpos=vd.antpos)
        new_vis.setup_data(self.new_bls, vd.times, vd.freqs, pol=vd.pol, data=data, history=vd.history)
        return new_vis


# ---------------------------------------------------------------------------------------
# redundant calibration: degeneracies (calibration.py:2611-2915); dense torch arithmetic on the input's device
# ---------------------------------------------------------------------------------------
def _lstsq_proj(A, wgts):
    """(A^T W A)^+ A^T W with W = diag(w / sum w), W = 1 without weights; A (N, 2)"""
    if wgts is None:
        return torch.pinverse(A.T @ A) @ A.T
    w = (wgts / torch.sum(wgts)).to(dtype=A.dtype, device=A.device)
    AtW = A.T * w
    return torch.pinverse(AtW @ A) @ AtW


def remove_redcal_degen(gains, ants, antpos, degen=None, wgts=None, redvis=None, bls=None, abs_amp=True, phs_slope=True):
    """
    Remove the redundant-calibration degeneracies from gains (Npol, Npol, Nants, Ntimes, Nfreqs; 1-pol or 2-pol) and, with
    redvis (Npol, Npol, Nbls, Ntimes, Nfreqs) and its baseline tuples bls, multiply them into the model visibilities
    (calibration.py:2611-2662): the degenerate gains are computed from the detached gains (wgts: 1-D antenna weights), divided
    by `degen` (a new degeneracy to insert) if given, and divided out of gains.  Returns (new_gains, new_vis | None,
    degen_gains).  The redvis branch runs through apply_cal and therefore needs GPU tensors; the rest works on any device.
    """
    rd = compute_redcal_degen(gains.detach(), ants, antpos, wgts=wgts, abs_amp=abs_amp, phs_slope=phs_slope)
    degen_gains = redcal_degen_gains(ants=ants, antpos=antpos, abs_amp=rd[0], phs_slope=rd[1])
    if degen is not None:
        degen_gains = degen_gains / degen
    new_gains = gains / degen_gains
    new_vis = None
    if redvis is not None:
        dg = degen_gains.to(redvis.device)
        if dg.shape[2] == 1 and len(ants) > 1:
            dg = dg.expand(dg.shape[:2] + (len(ants),) + dg.shape[3:])           # amplitude only: one gain for every antenna
        new_vis = apply_cal(redvis, bls, dg, ants, undo=False)[0]
    return new_gains, new_vis, degen_gains


def compute_redcal_degen(gains, ants, antpos, wgts=None, abs_amp=True, phs_slope=True):
    """
    The degeneracy parameters of redundant calibration of antenna gains (Npol, Npol, Nant, Ntimes, Nfreqs)
    (calibration.py:2665-2740): the overall amplitude eta = log sqrt(<|g|^2>), g_abs = exp(eta), of shape (Npol, Npol, 1,
    Ntimes, Nfreqs), and the phase gradient Phi [rad / m] over the array, g_phs = exp(i r . Phi), of shape (Npol, Npol, 2,
    Ntimes, Nfreqs) with (East, North) along axis 2, the (weighted) least-squares fit of the gain phases to the antenna
    positions.  wgts: 1-D antenna weights (default uniform).  Returns (abs_amp | None, phs_slope | None).
    """
    abs_amp_param = phs_slope_param = None
    if abs_amp:
        if wgts is None:
            abs_amp_param = torch.sum(torch.abs(gains) ** 2, dim=2, keepdim=True)
        else:
            w = wgts.to(gains.device)[:, None, None]
            abs_amp_param = torch.sum(torch.abs(gains) ** 2 * w, dim=2, keepdim=True) / torch.sum(w)
        abs_amp_param = torch.log(torch.sqrt(abs_amp_param))
    if phs_slope:
        gain_phs = torch.angle(gains)
        A = antpos[[a for a in ants]][:, :2].to(dtype=gain_phs.dtype, device=gains.device)
        phs_slope_param = torch.einsum("ab,ijblm->ijalm", _lstsq_proj(A, wgts), gain_phs)
    return abs_amp_param, phs_slope_param


def redcal_degen_gains(abs_amp=None, phs_slope=None, ants=None, antpos=None):
    """
    Degeneracy parameters (compute_redcal_degen) -> complex gains (Npol, Npol, Nant | 1, Ntimes, Nfreqs)
    (calibration.py:2743-2785).  The antenna axis follows `ants` (default: every antenna of antpos, which is what the reference
    always uses); antpos is needed for phs_slope.
    """
    device = abs_amp.device if abs_amp is not None else (phs_slope.device if phs_slope is not None else None)
    gains = torch.ones(1, 1, 1, 1, 1, dtype=utils._cfloat(), device=device)
    if abs_amp is not None:
        gains = gains * torch.exp(abs_amp)
    if phs_slope is not None:
        A = antpos[[a for a in (ants if ants is not None else antpos)]][:, :2].to(dtype=phs_slope.dtype, device=device)
        phs = (phs_slope.moveaxis(2, -1) @ A.T).moveaxis(-1, 2)
        gains = gains * torch.exp(1j * phs)
    return gains


def _bl_design(vd, bls, antpos):
    if isinstance(vd, dataset.VisData):
        bls, antpos = vd.bls, vd.antpos
    ant1, ant2 = zip(*bls)
    return (antpos[list(ant1)] - antpos[list(ant2)])[:, :2]


def compute_redcal_degen_vis(vd, wgts=None, abs_amp=True, phs_slope=True, bls=None, antpos=None):
    """
    The degeneracy parameters of a set of visibilities, a VisData or a tensor (Npol, Npol, Nbls, Ntimes, Nfreqs) with its
    baseline tuples bls and antpos (calibration.py:2788-2850): the log of the baseline-averaged amplitude, (Npol, Npol, 1,
    Ntimes, Nfreqs), and the phase gradient [rad / m] of the visibility phases over the baseline vectors r_1 - r_2,
    (Npol, Npol, 2, Ntimes, Nfreqs).  wgts: 1-D baseline weights.  The weighted branch of the reference names variables that
    do not exist and cannot run; this is the weighted least squares it plainly intends, W = diag(w / sum w).
    """
    data = vd.data if isinstance(vd, dataset.VisData) else vd
    abs_amp_param = phs_slope_param = None
    if abs_amp:
        if wgts is None:
            abs_amp_param = torch.sum(torch.abs(data), dim=2, keepdim=True)
        else:
            w = wgts.to(data.device)[:, None, None]
            abs_amp_param = torch.sum(torch.abs(data) * w, dim=2, keepdim=True) / torch.sum(w)
        abs_amp_param = torch.log(abs_amp_param)
    if phs_slope:
        vis_phs = torch.angle(data)
        A = _bl_design(vd, bls, antpos).to(dtype=vis_phs.dtype, device=data.device)
        phs_slope_param = torch.einsum("ab,ijblm->ijalm", _lstsq_proj(A, wgts), vis_phs)
    return abs_amp_param, phs_slope_param


def redcal_degen_vis(abs_amp=None, phs_slope=None, vd=None, bls=None, antpos=None):
    """
    Degeneracy parameters of visibilities (compute_redcal_degen_vis) -> the degenerate visibilities exp(abs_amp) *
    exp(i (r_1 - r_2) . Phi) (calibration.py:2853-2915): a tensor, or with vd a new VisData with vd's metadata (zeros when no
    parameter is given).  The reference decides which parameters are present by the truth value of the tensors, which only
    single-element tensors have; here a parameter is present when it is not None.
    """
    data = None
    if abs_amp is not None:
        data = torch.exp(abs_amp)
    if phs_slope is not None:
        A = _bl_design(vd, bls, antpos).to(dtype=phs_slope.dtype, device=phs_slope.device)
        phs_data = torch.exp(1j * (phs_slope.moveaxis(2, -1) @ A.T).moveaxis(-1, 2))
        data = phs_data if data is None else data * phs_data
    if vd is None:
        return data
    out = dataset.VisData()
    out.setup_meta(telescope=vd.telescope, antpos=vd.antpos)
    if data is None:
        data = torch.zeros_like(vd.data)
    out.setup_data(vd.bls, vd.times, vd.freqs, pol=vd.pol, data=data, flags=vd.flags, cov=vd.cov, cov_axis=vd.cov_axis,
                   icov=vd.icov, history=vd.history)
    return out


# ---------------------------------------------------------------------------------------
# vanilla models from a VisData (calibration.py:2918-2983)
# ---------------------------------------------------------------------------------------
def _param_sizes(vis, freq_mode, time_mode, freq_LM, time_LM):
    """(Ntime_params, Nfreq_params): the VisData's axes in channel mode, the LinearModel's feature count in linear mode"""
    Nt = vis.Ntimes if time_mode == 'channel' else int(time_LM.A.shape[1])
    Nf = vis.Nfreqs if freq_mode == 'channel' else int(freq_LM.A.shape[1])
    return Nt, Nf


def vis2JonesModel(vis, param_type='com', freq_mode='channel', time_mode='channel', freqs=None, freq_LM=None, time_LM=None,
                   refant=None, single_ant=False):
    """
    A vanilla JonesModel for a VisData (calibration.py:2918-2954): unit gains ('com', stored as a real view) or zero parameters,
    one per antenna of vis.bls (2 for the slope types, 1 with single_ant).  The reference sizes the time and channel axes from
    R.Ntime_params / R.Nfreq_params, which its response classes do not define in channel mode; here they are the VisData's
    Ntimes / Nfreqs in channel mode and the LinearModel's number of features (A.shape[1]) in linear mode.
    """
    R = JonesResponse(param_type=param_type, antpos=vis.antpos, freq_mode=freq_mode, freq_LM=freq_LM, freqs=freqs,
                      time_mode=time_mode, time_LM=time_LM)
    ants = sorted(int(a) for a in np.unique(np.asarray(vis.bls).ravel()))
    polmode = '1pol' if vis.Npol == 1 else '4pol'
    Nants = 2 if 'slope' in param_type else (1 if single_ant else len(ants))
    Nt, Nf = _param_sizes(vis, freq_mode, time_mode, freq_LM, time_LM)
    if param_type == 'com':
        params = utils.viewreal(torch.ones(vis.Npol, vis.Npol, Nants, Nt, Nf, dtype=utils._cfloat()))
    else:
        params = torch.zeros(vis.Npol, vis.Npol, Nants, Nt, Nf, dtype=utils._float())
    return JonesModel(params, ants=ants, R=R, refant=refant, polmode=polmode, single_ant=single_ant)


def vis2RedVisModel(vis, param_type='com', freq_mode='channel', time_mode='channel', freqs=None, freq_LM=None, time_LM=None,
                    redtol=1.0):
    """
    A vanilla RedVisModel for a VisData (calibration.py:2957-2983): zero parameters, one row per redundant group of vis.bls
    (telescope_model.build_reds with redtol).  Axis sizes as in vis2JonesModel: the VisData's in channel mode, the
    LinearModel's number of features in linear mode (the reference reads attributes its responses do not define).
    """
    reds, _, bl2red = telescope_model.build_reds(vis.antpos, bls=vis.bls, redtol=redtol)[:3]
    R = VisModelResponse(param_type=param_type, freq_mode=freq_mode, freqs=freqs, freq_LM=freq_LM, time_mode=time_mode,
                         time_LM=time_LM)
    Nt, Nf = _param_sizes(vis, freq_mode, time_mode, freq_LM, time_LM)
    params = torch.zeros(vis.Npol, vis.Npol, len(reds), Nt, Nf, dtype=utils._cfloat())
    if param_type == 'com':
        params = utils.viewreal(params)
    return RedVisModel(params, bl2red, R=R)
