"""
Minimal data containers with the reference's attribute layout: what RIME.forward emits
(`VisData`, dataset.py:289-411) and what sky models emit (`MapData`, dataset.py:1867-1936).
The tensor layout, the metadata fields and the index selection (`get_inds` / `get_data` / `get_cov`, what
imaging.VisMapper reads visibilities and weights through) are mirrored -- HDF5 IO, averaging etc. are outside
the hot path.
"""
import copy as _copy

import numpy as np
import torch

from . import utils


class TensorData:
    def __init__(self):
        self.data = None
        self.flags = None
        self.cov = None
        self.icov = None
        self.cov_axis = None
        self.cov_ndim = None
        self.cov_logdet = torch.tensor(0.0)

    def set_cov(self, cov, cov_axis, icov=None):
        """covariance (data-shaped variances for cov_axis None, a matrix for 'full', matrices along the last two axes
        otherwise) with the log-determinant and dimension the likelihood normalisation uses (dataset.py:70-124)"""
        logdet = None
        if isinstance(cov, torch.Tensor):
            if cov_axis is None:
                logdet = torch.sum(torch.log(cov))
            elif cov_axis == 'full':
                logdet = torch.slogdet(cov).logabsdet
            else:
                logdet = torch.slogdet(cov.reshape((-1,) + tuple(cov.shape[-2:]))).logabsdet.sum()
            if torch.is_complex(logdet):
                logdet = logdet.real
        elif isinstance(icov, torch.Tensor) and cov_axis is None:
            logdet = torch.sum(-torch.log(icov))
        self.cov = cov.clone() if isinstance(cov, torch.Tensor) else cov
        self.icov = icov.clone() if isinstance(icov, torch.Tensor) else icov
        self.cov_axis = cov_axis
        self.cov_ndim = int(np.prod(self.data.shape)) if self.data is not None else None
        self.cov_logdet = logdet if logdet is not None else torch.tensor(0.0)

    def compute_icov(self, inv='pinv', **kwargs):
        """compute the inverse covariance from self.cov and set it as self.icov (dataset.py:126-140); inv and kwargs:
        optim.compute_icov"""
        from . import optim
        self.icov = optim.compute_icov(self.cov, self.cov_axis, inv=inv, **kwargs)

    def get_data(self, **kwargs):
        return self.data

    def get_flags(self, **kwargs):
        return self.flags

    def get_cov(self, **kwargs):
        return self.cov

    def get_icov(self, **kwargs):
        return self.icov

    def push(self, device):
        for k in ('data', 'flags', 'cov', 'icov'):
            v = getattr(self, k, None)
            if isinstance(v, torch.Tensor):
                setattr(self, k, utils.push(v, device))


class VisData(TensorData):
    """visibilities of shape (Npol, Npol, Nbl, Ntimes, Nfreqs) + metadata (dataset.py:289)"""
    def __init__(self):
        super().__init__()
        self.atol = 1e-10
        self._file = None
        self.setup_meta()

    def setup_meta(self, telescope=None, antpos=None):
        self.telescope = telescope
        if antpos is not None and not isinstance(antpos, utils.AntposDict):
            antpos = utils.AntposDict(list(antpos.keys()), list(antpos.values()))
        self.antpos = antpos
        self.ants = antpos.ants if antpos is not None else None

    def setup_data(self, bls, times, freqs, pol=None, data=None, flags=None, cov=None,
                   cov_axis=None, icov=None, history='', file=None):
        self.data = data
        self._set_bls(bls)
        self.times = torch.as_tensor(times)
        self.Ntimes = len(times)
        self.freqs = torch.as_tensor(freqs)
        self.Nfreqs = len(freqs)
        self.pol = pol
        if isinstance(pol, str):
            assert pol.lower() in ['ee', 'nn'], "pol must be 'ee' or 'nn' for 1pol mode"
        self.Npol = 2 if pol is None else 1
        self.flags = flags
        self.set_cov(cov, cov_axis, icov=icov)
        self.history = history
        self._file = file

    def _set_bls(self, bls):
        if isinstance(bls, torch.Tensor):
            bls = bls.cpu().numpy()
        if isinstance(bls, np.ndarray) and bls.ndim == 1:
            self.blnums = bls
        else:
            self.blnums = np.asarray(utils.ants2blnum([tuple(b) for b in bls])) if len(bls) else np.array([])
        self._blnums = torch.as_tensor(self.blnums)
        self.Nbls = len(self.blnums)

    @property
    def bls(self):
        return utils.blnum2ants(self.blnums)

    def push(self, device, return_obj=False):
        super().push(device)
        self.freqs = utils.push(self.freqs, device)
        if return_obj:
            return self

    def copy(self, copydata=False, copymeta=False, detach=True):
        """new VisData sharing (or cloning) the tensors; copymeta re-instantiates telescope / antpos / axes, which
        drops the telescope's conversion cache (dataset.py:556-605)"""
        vd = VisData()
        telescope, antpos = self.telescope, self.antpos
        times, freqs, blnums = self.times, self.freqs, self.blnums
        flags, cov, icov, data = self.flags, self.cov, self.icov, self.data
        if copydata and data is not None:
            data = (data.detach() if (data.requires_grad and detach) else data).clone()
        if copymeta:
            if telescope is not None:
                telescope = telescope.__class__(telescope.location, tloc=getattr(telescope, 'tloc', None),
                                                device=telescope.device)
            if antpos is not None:
                antpos = antpos.__class__(_copy.deepcopy(antpos.ants), antpos.antvecs.clone())
            times, freqs, blnums = _copy.deepcopy(times), _copy.deepcopy(freqs), _copy.deepcopy(blnums)
            flags, cov, icov = [x.clone() if isinstance(x, torch.Tensor) else x for x in (flags, cov, icov)]
        vd.setup_meta(telescope=telescope, antpos=antpos)
        vd.setup_data(blnums, times, freqs, pol=self.pol, data=data, flags=flags, cov=cov, cov_axis=self.cov_axis,
                      icov=icov, history=self.history)
        return vd

    # ---- selection (dataset.py:607-1042): one fancy-indexed axis at most, everything else slices
    def _bl2ind(self, bl):
        if isinstance(bl, (list, np.ndarray, torch.Tensor)):
            if isinstance(bl, torch.Tensor):
                bl = bl.cpu().numpy()
            elif isinstance(bl, list):
                bl = utils.ants2blnum(bl)
            return [self._bl2ind(b) for b in bl]
        if isinstance(bl, tuple):
            bl = utils.ants2blnum(bl)
        idx = np.where(self.blnums == bl)[0]
        if len(idx) == 0:
            raise ValueError("Couldn't find bl {}".format(bl))
        return idx[0]

    def _time2ind(self, time, atol=None):
        if isinstance(time, (list, np.ndarray)) or (isinstance(time, torch.Tensor) and time.ndim == 1):
            return np.concatenate([self._time2ind(t, atol) for t in time]).tolist()
        atol = atol if atol is not None else self.atol          # rtol 1e-13: 0.03 s on a Julian date
        return np.where(np.isclose(np.asarray(self.times.cpu()), float(time), atol=atol, rtol=1e-13))[0].tolist()

    def _freq2ind(self, freq, atol=None):
        if isinstance(freq, (list, np.ndarray)) or (isinstance(freq, torch.Tensor) and freq.ndim == 1):
            return np.concatenate([self._freq2ind(f, atol) for f in freq]).tolist()
        atol = atol if atol is not None else self.atol
        return torch.where(torch.isclose(self.freqs, torch.as_tensor(freq, dtype=self.freqs.dtype,
                                                                     device=self.freqs.device), atol=atol))[0].tolist()

    def _pol2ind(self, pol, data=None):
        if isinstance(pol, list):
            assert len(pol) == 1
            pol = pol[0]
        assert isinstance(pol, str)
        if self.pol is not None:
            if pol.lower() != self.pol.lower():
                raise ValueError("cannot index pol from 1pol {}".format(self.pol))
            return (slice(0, 1), slice(0, 1))
        if pol.lower() == 'ee':
            return (slice(0, 1), slice(0, 1))
        if pol.lower() == 'nn':
            data = data if data is not None else self.data
            return (slice(1, 2), slice(0, 1)) if tuple(data.shape[:2]) == (2, 1) else (slice(1, 2), slice(1, 2))
        raise ValueError("only 'ee' / 'nn' can be indexed")

    def get_inds(self, bl=None, times=None, freqs=None, pol=None, bl_inds=None, time_inds=None, freq_inds=None,
                 data=None, atol=None):
        """5 index objects (pol, pol, bl, time, freq) for a selection by value or by index (dataset.py:776-862)"""
        data = data if data is not None else self.data
        if bl is not None:
            assert bl_inds is None
            bl_inds = self._bl2ind(bl)
        elif bl_inds is None:
            bl_inds = slice(None)
        if times is not None:
            assert time_inds is None
            time_inds = self._time2ind(times, atol=atol)
        elif time_inds is None:
            time_inds = slice(None)
        if freqs is not None:
            assert freq_inds is None
            freq_inds = self._freq2ind(freqs, atol=atol)
        elif freq_inds is None:
            freq_inds = slice(None)
        pol_inds = self._pol2ind(pol, data=data) if pol is not None else (slice(None), slice(None))
        inds = tuple(utils._list2slice(i) for i in (pol_inds[0], pol_inds[1], bl_inds, time_inds, freq_inds))
        assert sum(isinstance(i, slice) for i in inds) > 3, "cannot fancy index more than 1 axis"
        return inds

    def _take(self, x, squeeze, try_view, **sel):
        if x is None:
            return None
        inds = self.get_inds(data=x, **sel)
        x = x[inds]
        if not try_view and all(isinstance(i, slice) for i in inds):
            x = x.clone()
        return x.squeeze() if squeeze else x

    def get_data(self, bl=None, times=None, freqs=None, pol=None, bl_inds=None, time_inds=None, freq_inds=None,
                 squeeze=True, data=None, try_view=False, **kwargs):
        """slice of the data tensor (dataset.py:864-911)"""
        return self._take(self.data if data is None else data, squeeze, try_view, bl=bl, times=times, freqs=freqs,
                          pol=pol, bl_inds=bl_inds, time_inds=time_inds, freq_inds=freq_inds, **kwargs)

    def get_flags(self, bl=None, times=None, freqs=None, pol=None, bl_inds=None, time_inds=None, freq_inds=None,
                  squeeze=True, flags=None, try_view=False, **kwargs):
        return self._take(self.flags if flags is None else flags, squeeze, try_view, bl=bl, times=times, freqs=freqs,
                          pol=pol, bl_inds=bl_inds, time_inds=time_inds, freq_inds=freq_inds, **kwargs)

    def get_cov(self, bl=None, times=None, freqs=None, pol=None, bl_inds=None, time_inds=None, freq_inds=None,
                squeeze=True, cov=None, try_view=False, atol=None, **kwargs):
        """slice of the covariance (dataset.py:954-1035): data-shaped (cov_axis None) or one covariance matrix
        along the named axis"""
        cov = self.cov if cov is None else cov
        if cov is None:
            return None
        if self.cov_axis is None:
            return self._take(cov, squeeze, try_view, bl=bl, times=times, freqs=freqs, pol=pol, bl_inds=bl_inds,
                              time_inds=time_inds, freq_inds=freq_inds)
        if self.cov_axis == 'full':
            raise NotImplementedError
        inds = self.get_inds(bl=bl, times=times, freqs=freqs, pol=pol, bl_inds=bl_inds, time_inds=time_inds,
                             freq_inds=freq_inds, data=self.data)
        axis = self.cov_axis
        if bl is not None or bl_inds is not None:
            cov = cov[..., inds[2]][..., inds[2]] if axis == 'bl' else cov[:, :, inds[2]]
        elif times is not None or time_inds is not None:
            cov = (cov[..., inds[3]][..., inds[3]] if axis == 'time' else
                   (cov[:, :, inds[3]] if axis == 'bl' else cov[:, :, :, inds[3]]))
        elif freqs is not None or freq_inds is not None:
            cov = cov[..., inds[4]][..., inds[4]] if axis == 'freq' else cov[:, :, :, inds[4]]
        elif pol is not None:
            cov = cov[inds[0], inds[0]]
        if squeeze:
            cov = cov.squeeze()
        if not try_view and all(isinstance(i, slice) for i in inds):
            cov = cov.clone()
        return cov

    def get_icov(self, bl=None, icov=None, try_view=False, **kwargs):
        return self.get_cov(bl=bl, cov=self.icov if icov is None else icov, try_view=try_view, **kwargs)

    def bl_average(self, reds=None, wgts=None, redtol=1.0, inplace=False):
        """
        Average baselines together (dataset.py:1257-1361); baselines in no group of `reds` are dropped.  reds: list of
        baseline groups as antenna pairs or baseline numbers, e.g. [[(0, 1), (1, 2)], [(2, 5), (3, 6)]]; default: the
        redundant groups of self.antpos within redtol metres.  wgts: weights shaped like the data; default: self.icov
        when it holds inverse variances (cov_axis None), else uniform.  Flags, cov and icov are averaged along.
        inplace: edit this object, else return a new one.
        """
        if reds is None:
            from . import telescope_model
            red_info = telescope_model.build_reds(self.antpos, bls=self.bls, redtol=redtol)
            reds, bl2red = red_info[0], red_info[2]
        else:
            bl2red = {}
            for i, red in enumerate(reds):
                for bl in red:
                    bl2red[bl] = i
        bls = self.bls if isinstance(list(bl2red.keys())[0], tuple) else self.blnums
        Nmax = len(reds)
        index = torch.as_tensor([bl2red.get(bl, Nmax) for bl in bls], device=self.data.device)
        Nout_bls = index.unique().numel()
        truncate = bool((index == Nmax).any())
        if wgts is None and self.icov is not None and self.cov_axis is None:
            wgts = self.icov
        cov = None
        if self.cov_axis is None:
            if self.cov is not None:
                cov = self.cov
            elif self.icov is not None:
                cov = 1 / self.icov.clip(1e-60)
        avg_data, sum_wgts, avg_cov = average_data(self.data, -3, index, Nout_bls, wgts=wgts, cov=cov, truncate=truncate)
        avg_flags = None
        if self.flags is not None:
            shape = list(avg_data.shape[-self.flags.ndim:])
            if truncate:
                shape[-3] += 1
            # a group is flagged where all of its members are: count the unflagged members
            count = torch.zeros(shape, dtype=torch.int64, device=avg_data.device)
            count.index_add_(-3, index, (~self.flags).to(torch.int64))
            avg_flags = count == 0
            if truncate:
                avg_flags = avg_flags[..., :-1, :, :]
        avg_icov = None
        if self.icov is not None:
            avg_icov = 1 / avg_cov.clip(1e-60)
        if self.cov is None:
            avg_cov = None
        vout = self if inplace else self.copy(copydata=False, copymeta=False)
        vout.setup_data([red[0] for red in reds], vout.times, vout.freqs, pol=self.pol, data=avg_data, flags=avg_flags,
                        cov=avg_cov, icov=avg_icov, cov_axis=None, history=self.history)
        return vout

    # ---- LST alignment (dataset.py:1363-1566): rephasing, nearest-LST selection and time averaging on one fused kernel
    def get_bl_vecs(self, bls):
        """baseline vectors (Nbl, 3) in ENU [m] of antenna pairs or baseline numbers (dataset.py:534-554)"""
        if isinstance(bls, (np.ndarray, torch.Tensor)):
            ant1, ant2 = utils.blnum2ants(bls, separate=True)
        else:
            ant1, ant2 = zip(*bls)
        return self.antpos[list(ant2)] - self.antpos[list(ant1)]

    def _rephase_tau(self, dLST):
        from . import telescope_model
        dLST = np.asarray(utils.tensor2numpy(dLST) if isinstance(dLST, torch.Tensor) else dLST, dtype=np.float64)
        return telescope_model.rephase_tau(dLST, self.telescope.location[1], self.get_bl_vecs(self.bls))

    def lst_rephase(self, dtime=None, dLST=None, inplace=True):
        """
        Rephase zenith-pointing drift-scan data by a difference in LST (dataset.py:1363-1399).  dLST [rad]: a scalar or one
        value per time.  dtime [Julian days] (parity unpinned: the reference takes the sidereal day from astropy, here
        SDAY_SEC = 86164.0905 s): converted as dLST = dtime 2 pi / sidereal day.  The delay of every (baseline, time) is
        computed on the host; the phasor is generated and applied inside one launch (ops.vis_timeavg with singleton bins),
        never stored.  Differentiable with respect to the data.  inplace: this object receives the rephased tensor.
        """
        from . import ops
        if dLST is None:
            assert dtime is not None
            dLST = np.asarray(utils.tensor2numpy(dtime) if isinstance(dtime, torch.Tensor) else dtime,
                              dtype=np.float64) * 2 * np.pi / (SDAY_SEC / 86400.0)
        tau = self._rephase_tau(dLST)
        if tau.shape[1] != self.Ntimes:
            tau = tau.expand(tau.shape[0], self.Ntimes)
        plan = ops.TimeAvgPlan(np.arange(self.Ntimes)[:, None], self.Ntimes)
        vd = self if inplace else self.copy(copydata=False)
        vd.data = ops.vis_timeavg(self.data, plan, tau=tau, freqs=self.freqs)[0]
        return vd

    def time_nn_interp(self, lsts, rephase=True, inplace=True):
        """
        Nearest-neighbour interpolation onto the LST bins `lsts` [rad] (dataset.py:1401-1450): every target takes the
        integration whose LST is nearest (both LST sets unwrapped across 2 pi by the reference's rule) and, with rephase,
        is rephased by the remaining difference -- one launch with singleton bins, in which data, flags and cov follow the
        selected times (icov by a plain gather); `times` becomes the selected times.  An integration may serve several
        targets, each with its own delay.  Differentiable with respect to the data.
        """
        from . import ops, telescope_model
        lsts = np.array(utils.tensor2numpy(lsts) if isinstance(lsts, torch.Tensor) else lsts, dtype=np.float64)
        t_idx, dLST = nearest_lst(lsts, telescope_model.JD2LST(utils.tensor2numpy(self.times), self.telescope.location[0]) * utils.D2R)
        plan = ops.TimeAvgPlan(t_idx[:, None], self.Ntimes)
        tau = self._rephase_tau(dLST) if rephase else None
        diag = self.cov_axis is None
        data, _, cov, flags = ops.vis_timeavg(self.data, plan, cov=self.cov if diag else None, flags=self.flags, tau=tau,
                                              freqs=self.freqs, tau_by_member=True)
        icov = self.icov
        if not diag:
            cov = self.get_cov(time_inds=t_idx.tolist(), squeeze=False) if self.cov is not None else None
            icov = self.get_icov(time_inds=t_idx.tolist(), squeeze=False) if self.icov is not None else None
        elif icov is not None:
            icov = icov.index_select(-2, torch.as_tensor(t_idx, device=icov.device))
        vd = self if inplace else self.copy(copydata=False)
        vd.setup_data(self.blnums, self.times[torch.as_tensor(t_idx)], self.freqs, pol=self.pol, data=data, flags=flags, cov=cov,
                      cov_axis=self.cov_axis, icov=icov, history=self.history)
        return vd

    def time_average(self, time_inds=None, wgts=None, rephase=False, inplace=True):
        """
        Average time integrations together (dataset.py:1452-1566).  time_inds: list of index sequences into self.times,
        one per output time (default: all times into one); a time in no entry is dropped, a time in several goes to the
        last (the reference's rule).  wgts: weights; default self.icov when it holds inverse variances (cov_axis None),
        else uniform.  rephase: rephase every member to the mean time of its bin (drift-scan data) before averaging.
        Averaged times are the plain mean of the members; flags (set where every member is flagged), cov and icov
        (1 / avg_cov.clip(1e-60); cov kept only if it was set) follow the reference.
        Weights of the data's full shape (or none) with a diagonal covariance go through one launch of the fused kernel
        (ops.vis_timeavg: phasor, weighting, the sums of data, weights and variances and the flags; fixed summation order,
        bit-identical from run to run); any other input goes through average_data.  Differentiable with respect to the data
        only: weights, times and cov receive no gradient.
        """
        from . import ops, telescope_model
        Nt = self.Ntimes
        if time_inds is None:
            time_inds = [np.arange(Nt)]
        Nbin = len(time_inds)
        bins, index = time_bins(time_inds, Nt)
        if wgts is None and self.icov is not None and self.cov_axis is None:
            wgts = self.icov
        cov = None
        if self.cov_axis is None:
            if self.cov is not None:
                cov = self.cov
            elif self.icov is not None:
                cov = 1 / self.icov.clip(1e-60)
        times = utils.tensor2numpy(self.times).astype(np.float64)
        avg_times = np.array([times[b].mean() if len(b) else np.nan for b in bins])
        tau = None
        if rephase:
            dtimes = np.where(index < Nbin, np.append(avg_times, 0.0)[index] - times, 0.0)
            tau = self._rephase_tau(dtimes * 2 * np.pi / (SDAY_SEC / 86400.0))
        if self.cov_axis is None and (wgts is None or tuple(wgts.shape) == tuple(self.data.shape)):
            avg_data, _, avg_cov, avg_flags = ops.vis_timeavg(self.data, ops.TimeAvgPlan(bins, Nt), wgts=wgts, cov=cov,
                                                              flags=self.flags, tau=tau, freqs=self.freqs)
        else:
            data = self.data
            if tau is not None:
                data = data * ops.rephase_phasor(tau.to(data.device), self.freqs, dtype=data.dtype)
            truncate = bool((index == Nbin).any())
            idx = torch.as_tensor(index, device=data.device)
            avg_data, _, avg_cov = average_data(data, -2, idx, Nbin + int(truncate), wgts=wgts, cov=cov, truncate=truncate)
            avg_flags = None
            if self.flags is not None:
                shape = list(avg_data.shape[-self.flags.ndim:])
                shape[-2] = Nbin + 1
                count = torch.zeros(shape, dtype=torch.int64, device=data.device)
                count.index_add_(-2, idx, (~self.flags).to(torch.int64))
                avg_flags = (count == 0)[..., :Nbin, :]
        avg_icov = None
        if self.icov is not None and avg_cov is not None:
            avg_icov = 1 / avg_cov.clip(1e-60)
        if self.cov is None:
            avg_cov = None
        vout = self if inplace else self.copy(copydata=False, copymeta=False)
        vout.setup_data(self.blnums, torch.as_tensor(avg_times), vout.freqs, pol=self.pol, data=avg_data, flags=avg_flags,
                        cov=avg_cov, icov=avg_icov, cov_axis=None, history=self.history)
        return vout

    def _inflate_by_redundancy(self, new_bls, red_bl_inds, try_view=False):
        """
        new VisData whose baseline axis is self's indexed by red_bl_inds (one redundant-group index per
        baseline of new_bls): data, flags, cov and icov alike (dataset.py:1568-1602).  The gather is a
        differentiable index_select on the tensors' own device.
        """
        idx = torch.as_tensor(red_bl_inds, dtype=torch.int64)

        def take(x):
            if x is None:
                return None
            return x.index_select(2, idx.to(x.device))

        cov = self.cov if (self.cov is None or self.cov_axis not in (None, 'bl')) else take(self.cov)
        icov = self.icov if (self.icov is None or self.cov_axis not in (None, 'bl')) else take(self.icov)
        out = VisData()
        out.setup_meta(telescope=self.telescope, antpos=self.antpos)
        out.setup_data(new_bls, self.times, self.freqs, pol=self.pol, data=take(self.data), flags=take(self.flags),
                       cov=cov, cov_axis=self.cov_axis, icov=icov, history=self.history)
        return out

    def inflate_by_redundancy(self, bls, bl2red):
        """copy every redundant type held here over to the physical baselines `bls` of the same type
        (bl2red: baseline -> redundant-group index, e.g. ArrayModel.bl2red; dataset.py:1604-1640)"""
        mine = {bl2red[b]: i for i, b in enumerate(self.bls)}
        keep = [b for b in bls if bl2red[b] in mine]
        return self._inflate_by_redundancy(keep, [mine[bl2red[b]] for b in keep])



SDAY_SEC = 86164.0905        # mean sidereal day [s] (the reference takes astropy.units.sday)


def time_bins(time_inds, Nt):
    """(bins, index) of VisData.time_average: index [Nt], the bin of every time by the reference's rule (a time listed in
    several entries goes to the last; len(time_inds) marks a time in none, which is dropped) and bins, the ascending times of
    every entry -- an empty entry is an empty bin.  Host numpy."""
    Nbin = len(time_inds)
    index = np.full(int(Nt), Nbin, dtype=np.int64)
    for i, tinds in enumerate(time_inds):
        tinds = np.asarray(tinds.cpu() if isinstance(tinds, torch.Tensor) else tinds)
        if isinstance(tinds, np.ndarray) and tinds.dtype == object:
            raise ValueError('time_inds entries must be integer sequences')
        tinds = tinds.reshape(-1).astype(np.int64) if tinds.size else np.zeros(0, dtype=np.int64)
        if tinds.size and (tinds.min() < -Nt or tinds.max() >= Nt):
            raise IndexError('time index outside the %d times' % Nt)
        index[tinds] = i
    return [np.where(index == i)[0] for i in range(Nbin)], index


def nearest_lst(lsts, self_lsts):
    """(t_idx, dLST) of VisData.time_nn_interp by the reference's rule (dataset.py:1421-1438): both LST sets [rad] are
    unwrapped across 2 pi (values below the first get 2 pi added when the last lies below the first), the targets are
    lifted by 2 pi when they start below the data, every target takes the nearest data LST (the first of equals), and
    dLST = target - selected.  Copies: the inputs are left as they are."""
    lsts, self_lsts = np.array(lsts, dtype=np.float64).reshape(-1), np.array(self_lsts, dtype=np.float64).reshape(-1)
    if lsts[-1] < lsts[0]:
        lsts[lsts < lsts[0]] += 2 * np.pi
    if self_lsts[-1] < self_lsts[0]:
        self_lsts[self_lsts < self_lsts[0]] += 2 * np.pi
    if lsts[0] < self_lsts[0]:
        lsts += 2 * np.pi
    t_idx = np.argmin(np.abs(self_lsts - lsts[:, None]), axis=1)
    return t_idx, lsts - self_lsts[t_idx]


def average_data(data, dim, index, N, wgts=None, cov=None, truncate=False):
    """
    Weighted average of a tensor along `dim` with torch.index_add_ (dataset.py:3940-4052): index[i] is the output slot
    of element i along dim, N the number of slots, e.g. [0, 1, 0, 1] -> [mean(data[[0, 2]]), mean(data[[1, 3]])].
    wgts: weights that broadcast against data (uniform when None); cov: variances of the data (its trailing axes),
    propagated through the weighted sum; truncate: drop the last slot, the one that collects the elements no output needs.
    Returns (avg_data, sum_wgts, avg_cov); avg_cov = sum w^2 cov / (sum w)^2, which is 1 / sum w for w = 1 / cov.
    """
    dim = int(np.arange(-data.ndim, 0, 1)[dim])
    if wgts is None:
        shape = [1] * data.ndim
        shape[dim] = data.shape[dim]
        wgts = torch.ones(shape, device=data.device, dtype=data.real.dtype if data.is_complex() else data.dtype)   # the reference: default dtype
    if wgts.shape[dim] != data.shape[dim]:
        shape = list(wgts.shape)
        shape[dim] = data.shape[dim]
        wgts = wgts.expand(shape)
    shape = list(data.shape)
    shape[dim] = N
    avg_data = torch.zeros(shape, dtype=data.dtype, device=data.device)
    shape = list(wgts.shape)
    shape[dim] = N
    sum_wgts = torch.zeros(shape, dtype=wgts.dtype, device=wgts.device)
    sum_wgts.index_add_(dim, index, wgts)
    avg_data.index_add_(dim, index, data * wgts)
    avg_data = avg_data / sum_wgts.clip(1e-40)
    if cov is not None:
        assert cov.shape == data.shape[-cov.ndim:]
        shape = list(cov.shape)
        shape[dim] = N
        avg_cov = torch.zeros(shape, dtype=cov.dtype, device=cov.device)
        avg_cov.index_add_(dim, index, cov * wgts.pow(2))
        avg_cov = avg_cov / sum_wgts.clip(1e-40).pow(2)
    else:
        avg_cov = None
    if truncate:
        slices = [slice(None)] * data.ndim
        slices[dim] = slice(0, N - 1)
        avg_data = avg_data[tuple(slices)]
        sum_wgts = sum_wgts[tuple(slices[-wgts.ndim:])]
        if cov is not None:
            avg_cov = avg_cov[tuple(slices[-cov.ndim:])]
    return avg_data, sum_wgts, avg_cov


class RedVisAvg(utils.Module):
    """VisData redundant-averaging block of a forward-model chain (dataset.py:3651-3696): VisData.bl_average with the
    groups `reds`, the weights `wgts` (diagonal covariances only) and `inplace` fixed at construction; the counterpart of
    RedVisInflate and of calibration.PartialRedVisInflate"""
    def __init__(self, reds, wgts=None, inplace=False, device=None):
        super().__init__()
        self.reds = reds
        self.wgts = wgts
        self.inplace = inplace
        self.device = device

    def __call__(self, vd, **kwargs):
        return vd.bl_average(reds=self.reds, wgts=self.wgts, inplace=self.inplace)

    def forward(self, vd, **kwargs):
        return self(vd, **kwargs)

    def push(self, device):
        self.wgts = utils.push(self.wgts, device)
        if not isinstance(device, torch.dtype):
            self.device = device


class RedVisInflate(utils.Module):
    """VisData redundant-inflation block of a forward-model chain (dataset.py:3699-3735): the step that
    follows RIME when only one baseline per redundant group was simulated"""
    def __init__(self, new_bls, red_bl_inds):
        super().__init__()
        self.new_bls = new_bls
        self.red_bl_inds = torch.as_tensor(red_bl_inds, dtype=torch.int64)
        self.device = None

    def __call__(self, vd, **kwargs):
        return vd._inflate_by_redundancy(new_bls=self.new_bls, red_bl_inds=self.red_bl_inds)

    def forward(self, vd, **kwargs):
        return self(vd, **kwargs)

    def push(self, device):
        if not isinstance(device, torch.dtype):
            self.red_bl_inds = utils.push(self.red_bl_inds, device)
            self.device = device


class MapData(TensorData):
    """sky map of shape (Npol, 1, Nfreqs, Npix) with pixel angles (dataset.py:1867)"""
    def __init__(self):
        super().__init__()
        self.atol = 1e-10
        self.setup_meta()

    def setup_meta(self, name=None):
        self.name = name

    def setup_data(self, freqs, df=None, pols=None, data=None, angs=None, flags=None, cov=None,
                   cov_axis=None, icov=None, norm=None, history=''):
        self.freqs = freqs
        self.df = df
        self.angs = angs
        self.pols = pols
        self.data = data
        self.flags = flags
        self.norm = norm
        self.set_cov(cov, cov_axis, icov=icov)
        self.history = history


def concat_VisData(vds, axis):
    """concatenate VisData along 'bl' or 'time' (dataset.py:3739), metadata from the first"""
    assert axis in ('bl', 'time')
    out = VisData()
    out.setup_meta(vds[0].telescope, vds[0].antpos)
    if axis == 'bl':
        data = torch.cat([v.data for v in vds], dim=2)
        bls = utils.flatten([v.bls for v in vds])
        times = vds[0].times
    else:
        data = torch.cat([v.data for v in vds], dim=3)
        bls = vds[0].bls
        times = torch.cat([torch.as_tensor(v.times) for v in vds])
    out.setup_data(bls, times, vds[0].freqs, pol=vds[0].pol, data=data, history=vds[0].history)
    return out


def pass_data(obj, copy=False, **kwargs):
    """read function of an in-memory Dataset (dataset.py:4127-4133)"""
    import copy as _c
    return _c.deepcopy(obj) if copy else obj


class Dataset(torch.utils.data.Dataset):
    """the minibatches of target (or input) data a LogProb iterates over, one data object per batch
    (dataset.py:3611-3648); objects held in memory unless a read function is given"""
    def __init__(self, data, read_fn=None, read_kwargs={}):
        if isinstance(data, (str, TensorData)):
            data = [data]
        self.data = data
        self.Ndata = len(data)
        self.read_fn = read_fn if read_fn is not None else pass_data
        self.read_kwargs = [read_kwargs for _ in data] if isinstance(read_kwargs, dict) else read_kwargs

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        return self.read_fn(self.data[idx], **self.read_kwargs[idx])
