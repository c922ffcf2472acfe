"""
Fourier transforms along one axis: the reference's fft.py restated on one HIP kernel.

`FFT` is the windowed transform of a tensor or of a `dataset.VisData` / `MapData` along one axis (along frequency: the
delay transform), `PeakDelay` the delay of each line's peak by Quinn's second estimator, `vis_wedge` the redundantly
averaged delay transform of a VisData, `gen_window` the window functions.  Signatures, attribute names and defaults follow
the reference (fft.py:11-302).

Every application is ONE launch of `rime_fft_apply` (ops.fft_apply): window, ifftshift, transform, norm, fftshift, abs,
peak normalisation and |.|^2 happen between one load and one store of each line, where the reference runs a chain of
full passes over the tensor (fft.py:111-137); PeakDelay's estimate is an epilogue of the same launch, where the
reference calls `get_peak` once per line from a recursive Python loop (fft.py:175-182).  The data must be on the GPU;
there is no CPU path.  A gradient flows to the input through the linear part (the adjoint runs on the same kernel) and,
when one is asked for, abs / peak normalisation / square are the reference's torch expressions on the kernel's complex
spectrum.  PeakDelay is not differentiable.

Left out: transforms longer than 4096 samples, gradients to the window through the kernel (a window that requires grad
is multiplied in torch), a differentiable PeakDelay, N-dimensional transforms, CalData.
"""
import copy as _copy

import numpy as np
import torch

from . import utils, dataset, ops


class FFT(utils.Module):
    """A 1-D FFT block for tensors, VisData or MapData (fft.py:11-143)"""
    def __init__(self, dim=0, abs=False, peaknorm=False, N=None, dx=None, ndim=None, window=None, fftshift=True, ifft=False,
                 norm=None, edgecut=None, square=False, device=None, **kwargs):
        """
        dim: axis of the transform; abs / peaknorm / square: take |.|, divide each line by its max |.|, take |.|^2, in that
        order; N, dx: number of samples and their spacing (for .freqs and for a named window); ndim: number of axes of the
        inputs (for a named window); window: a name for gen_window (kwargs go there) or a tensor that broadcasts against
        the input; fftshift: fftshift after the fft, ifftshift BEFORE the ifft; ifft: the inverse transform; norm:
        'forward', 'backward' or 'ortho' as in torch.fft; edgecut: samples of zero weight at (start, end) of the axis, the
        named window spans the samples between them.
        """
        super().__init__()
        self.dim = dim
        self.abs = abs
        self.peaknorm = peaknorm
        self.dx = dx if dx is not None else 1.0
        self.fftshift = fftshift
        self.ifft = ifft
        self.norm = norm
        self.square = square
        self.device = None
        if N is not None:
            self.freqs = torch.fft.fftfreq(N, d=self.dx)
            if fftshift:
                self.freqs = torch.fft.fftshift(self.freqs)
            self.start = self.freqs[0]
            self.df = self.freqs[1] - self.freqs[0] if N > 1 else torch.as_tensor(1.0 / self.dx)
        else:
            self.start = 0.0
            self.dx, self.freqs, self.df = None, None, None
        if isinstance(edgecut, (int, np.integer)):
            edgecut = (edgecut, edgecut)
        elif edgecut is None:
            edgecut = (0, 0)
        self.edgecut = edgecut
        self.window = window
        self.win = None
        if window is not None:
            if isinstance(window, torch.Tensor):
                self.win = window
            else:
                assert N is not None
                assert ndim is not None
                win = gen_window(window, N - self.edgecut[0] - self.edgecut[1], **kwargs)
                win = torch.cat([torch.zeros(self.edgecut[0]), win, torch.zeros(self.edgecut[1])])
                shape = [1 for i in range(ndim)]
                shape[dim] = N
                self.win = win.reshape(*shape)
        if device is not None:
            self.push(device)

    def push(self, device):
        """move the window to a device, or re-type it (a dtype); plans are rebuilt on the next call"""
        if not isinstance(device, torch.dtype):
            self.device = device
        if isinstance(self.win, torch.Tensor):
            self.win = utils.push(self.win, device)
        self.__dict__.pop('_plans', None)

    def __getstate__(self):
        # pickle / deepcopy: the twiddle tables are derived from N; the copy builds them again on first use
        state = dict(self.__dict__)
        state.pop('_plans', None)
        return state

    def _plan(self, x):
        rdt = x.real.dtype if x.is_complex() else x.dtype
        key = (int(x.shape[self.dim]), rdt, str(x.device))
        plans = self.__dict__.setdefault('_plans', {})
        if key not in plans:
            plans[key] = ops.FFTPlan(key[0], rdt, x.device)
        return plans[key]

    def _epilogue(self):
        names = [n for n, on in (('abs', self.abs), ('peaknorm', self.peaknorm), ('square', self.square)) if on]
        return '+'.join(names) if names else 'none'

    def _kernel_window(self, inp, win):
        """(input, window vector): a real window along self.dim alone goes into the kernel, any other is multiplied here"""
        win = win if win is not None else self.win
        if win is None:
            return inp, None
        win = torch.as_tensor(win)
        d = self.dim % inp.ndim - (inp.ndim - win.ndim)
        N = inp.shape[self.dim]
        if (0 <= d < win.ndim and win.shape[d] == N == win.numel() and not win.is_complex() and win.is_floating_point()
                and not win.requires_grad):
            return inp, win.reshape(N)
        return inp * win.to(inp.device), None

    def _prepare(self, inp):
        if isinstance(inp, np.ndarray):
            inp = torch.as_tensor(inp)
        if self.device is not None and not inp.is_cuda:
            inp = inp.to(self.device)
        if not inp.is_complex() and inp.dtype not in (torch.float32, torch.float64):
            inp = inp.to(utils._float())
        return inp

    def forward(self, inp, ifft=None, win=None, **kwargs):
        """the transform of a tensor or numpy array; a VisData / MapData gives a copy with its data replaced"""
        if isinstance(inp, dataset.TensorData):
            out = _copy_data(inp)
            out.data = self.forward(inp.data, ifft=ifft, win=win, **kwargs)
            return out
        inp = self._prepare(inp)
        inp, win = self._kernel_window(inp, win)
        ifft = ifft if ifft is not None else self.ifft
        return ops.fft_apply(inp, self._plan(inp), dim=self.dim, inverse=bool(ifft), window=win, shift=bool(self.fftshift),
                             norm=self.norm, epilogue=self._epilogue())


class PeakDelay(FFT):
    """
    The peak delay along dim by Quinn's second estimator (fft.py:146-202): the first index n of the maximum of |y| along
    each line of the FFT block's output y (after the shift, and after abs / peaknorm / square when set), refined by the
    ratios real(y[n+1] / y[n]) and real(y[n-1] / y[n]) with neighbours that wrap round, returned as start + bin * df.
    One kernel launch for all lines.  Needs N (and dx) for start and df.  Not differentiable: the result carries no graph.
    """
    def __init__(self, **kwargs):
        super().__init__(**kwargs)

    def k(self, x):
        return 0.25 * torch.log(3 * x**2 + 6 * x + 1) \
            - np.sqrt(6) / 24 * torch.log((x + 1 - np.sqrt(2. / 3.)) / (x + 1 + np.sqrt(2. / 3.)))

    def forward(self, inp):
        if isinstance(inp, dataset.TensorData):
            out = _copy_data(inp)
            out.data = self.forward(inp.data)
            return out
        if self.df is None:
            raise ValueError('PeakDelay needs N (and dx) at construction: the peak is returned as start + bin * df')
        inp = self._prepare(inp)
        inp, win = self._kernel_window(inp, None)
        epi = self._epilogue()
        out = ops.fft_apply(inp, self._plan(inp), dim=self.dim, inverse=bool(self.ifft), window=win, shift=bool(self.fftshift),
                            norm=self.norm, epilogue='peak' if epi == 'none' else epi + '+peak', start=float(self.start),
                            df=float(self.df))
        return out.to(utils._float())


def _copy_data(obj):
    """a copy of a data container sharing its tensors (VisData.copy; a shallow copy for the containers without one)"""
    return obj.copy() if hasattr(obj, 'copy') else _copy.copy(obj)


def vis_wedge(vd, ravg_kwgs=None, **kwargs):
    """
    Average the redundant baseline groups of a VisData (ravg_kwgs go to VisData.bl_average) and take its FFT along
    frequency to form a wedge (fft.py:205-238); kwargs go to FFT.  Returns (VisData, the FFT object, whose .freqs are
    the delays).
    """
    ravg_kwgs = ravg_kwgs if ravg_kwgs is not None else {}
    vd = vd.bl_average(inplace=False, **ravg_kwgs)
    dfreq = vd.freqs[1] - vd.freqs[0]
    FT = FFT(dim=4, ndim=5, dx=float(dfreq), N=vd.Nfreqs, **kwargs)
    vd = FT(vd)
    return vd, FT


def _general_cosine(N, a):
    """sum_k a_k cos(k t), t from -pi to pi in N samples: scipy.signal.windows.general_cosine, symmetric form"""
    if N <= 1:
        return np.ones(max(N, 0))
    fac = np.linspace(-np.pi, np.pi, N)
    w = np.zeros(N)
    for k in range(len(a)):
        w += a[k] * np.cos(k * fac)
    return w


def _tukey(N, alpha):
    """tapered cosine window, symmetric form (scipy.signal.windows.tukey)"""
    if N <= 1:
        return np.ones(max(N, 0))
    if alpha <= 0:
        return np.ones(N)
    if alpha >= 1.0:
        return _general_cosine(N, [0.5, 0.5])
    n = np.arange(0, N)
    width = int(np.floor(alpha * (N - 1) / 2.0))
    n1, n2, n3 = n[0:width + 1], n[width + 1:N - width - 1], n[N - width - 1:]
    w1 = 0.5 * (1 + np.cos(np.pi * (-1 + 2.0 * n1 / alpha / (N - 1))))
    w3 = 0.5 * (1 + np.cos(np.pi * (-2.0 / alpha + 1 + 2.0 * n3 / alpha / (N - 1))))
    return np.concatenate((w1, np.ones(n2.shape), w3))


# coefficients of the 7-, 9- and 11-term cosine sums as the reference lists them (fft.py:273-289;
# https://ieeexplore.ieee.org/document/293419, https://ieeexplore.ieee.org/document/940309)
_BH4 = [0.35875, 0.48829, 0.14128, 0.01168]
_BH7 = [0.27105140069342, 0.43329793923448, 0.21812299954311, 0.06592544638803, 0.01081174209837, 0.00077658482522,
        0.00001388721735]
_CS9 = [2.384331152777942e-1, 4.00554534864382e-1, 2.358242530472107e-1, 9.527918858383112e-2, 2.537395516617152e-2,
        4.152432907505835e-3, 3.68560416329818e-4, 1.38435559391703e-5, 1.161808358932861e-7]
_CS11 = [2.151527506679809e-1, 3.731348357785249e-1, 2.424243358446660e-1, 1.166907592689211e-1, 4.077422105878731e-2,
         1.000904500852923e-2, 1.639806917362033e-3, 1.651660820997142e-4, 8.884663168541479e-6, 1.938617116029048e-7,
         8.482485599330470e-10]


def gen_window(window, N, alpha=None, edgecut=None, **kwargs):
    """
    A window function of N samples in the default real dtype (fft.py:241-302), symmetric form: 'none' / 'boxcar' /
    'tophat', 'blackmanharris' / 'bh' / 'bh4', 'hann' / 'hanning', 'tukey' (alpha: the tapered fraction, 0.5 when not
    given), 'gaussian' (alpha: the standard deviation in samples), 'bh7', 'cs9', 'cs11' (7-, 9- and 11-term cosine sums).
    edgecut = (start, end): that many zeros at the ends, the window spans the N - start - end samples between them.
    Any other name is looked up in scipy.signal.windows when SciPy is installed.
    """
    if edgecut is not None:
        N = N - sum(edgecut)
    if window in ['none', None, 'None', 'boxcar', 'tophat']:
        w = np.ones(N)
    elif window in ['blackmanharris', 'blackman-harris', 'bh', 'bh4']:
        w = _general_cosine(N, _BH4)
    elif window in ['hanning', 'hann']:
        w = _general_cosine(N, [0.5, 0.5])
    elif window == 'tukey':
        w = _tukey(N, 0.5 if alpha is None else alpha)
    elif window == 'gaussian':
        if alpha is None:
            raise ValueError("the 'gaussian' window needs its standard deviation: alpha")
        n = np.arange(0, N) - (N - 1.0) / 2.0
        w = np.exp(-n ** 2 / (2 * alpha * alpha))
    elif window in ['blackmanharris-7term', 'blackman-harris-7term', 'bh7']:
        w = _general_cosine(N, _BH7)
    elif window in ['cosinesum-9term', 'cosinesum9term', 'cs9']:
        w = _general_cosine(N, _CS9)
    elif window in ['cosinesum-11term', 'cosinesum11term', 'cs11']:
        w = _general_cosine(N, _CS11)
    else:
        try:
            from scipy.signal import windows
            w = getattr(windows, window)(N, **kwargs)
        except (ImportError, AttributeError, TypeError):
            raise ValueError("Didn't recognize window {}".format(window))
    if edgecut is not None:
        w = np.concatenate([np.zeros(edgecut[0]), w, np.zeros(edgecut[1])])
    return torch.as_tensor(w, dtype=utils._float())
