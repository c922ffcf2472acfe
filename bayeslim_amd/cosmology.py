"""
Cosmology conversions for 21 cm intensity mapping and the sampling of simulation boxes onto a lightcone
(reference cosmology.py).

`Cosmology` is the flat LambdaCDM model the reference obtains from astropy.cosmology.FlatLambdaCDM (Tcmb0 = 2.725 K,
Neff = 3.05, m_nu = [0, 0, 0.06] eV), written out here in float64 numpy: photons from the Stefan-Boltzmann law, the
neutrino temperature 0.7137658555036082 Tcmb0 and the massive-neutrino fitting function of Komatsu et al. 2011 (eq. 26) as
astropy states them.  PARITY UNPINNED against astropy itself (it is not available where this was written): the formulae
and constants (CODATA 2018) are the published ones, the closed forms and an independent quadrature are tested, no number
was compared with astropy's output.

`cube2lcone` / `cube2map` keep the reference's signatures and meaning and run on ONE launch of csrc/lcone.hip
(ops.lcone_sample) for all radii and pixels: the host (numpy float64) prepares the unit vectors and the radial stencil table,
the kernel gathers.  There is no CPU path.
"""
import numpy as np
import torch

from . import ops

# CODATA 2018 (exact SI values but G) and the IAU parsec
_C = 299792458.0                     # m / s
_G = 6.6743e-11                      # m^3 / kg / s^2
_KB = 1.380649e-23                   # J / K
_H = 6.62607015e-34                  # J s
_EV = 1.602176634e-19                # J
_SIGMA_SB = 2 * np.pi ** 5 * _KB ** 4 / (15 * _H ** 3 * _C ** 2)     # W / m^2 / K^4
_MPC = 3.0856775814913673e22         # m
_KB_EV = _KB / _EV                   # eV / K

_GL_ORDER = 64
_GL_X, _GL_W = np.polynomial.legendre.leggauss(_GL_ORDER)


class Distance(np.ndarray):
    """a plain float64 array of distances [Mpc] with the `.value` of an astropy Quantity, so that the reference's call
    sites (`cosmo.comoving_distance(z).value`) work unchanged"""

    @property
    def value(self):
        a = np.asarray(self)
        return a if a.ndim else a[()]


class Cosmology:
    """
    Flat LambdaCDM with the reference's additional methods for 21 cm intensity mapping.  Default parameters: Planck 2015.
    Radiation (photons and three neutrino species, one of 0.06 eV) is included as astropy includes it:
        Ogamma0 = 4 sigma Tcmb0^4 / (c^3 rho_crit0),   Tnu0 = 0.7137658555036082 Tcmb0,
        nu_rel(z) = 0.22710731766 (Neff / 3) sum_species (1 + (0.3173 y)^1.83)^(1 / 1.83),  y = m_nu / (k_B Tnu0 (1 + z)),
        Onu0 = Ogamma0 nu_rel(0),   Ode0 = 1 - Om0 - Ogamma0 - Onu0,
        E^2(z) = Om0 (1 + z)^3 + Ogamma0 (1 + nu_rel(z)) (1 + z)^4 + Ode0.
    """

    def __init__(self, H0=67.7, Om0=0.3075, Ob0=0.0486):
        """
        H0 : Hubble parameter at z = 0 [km / s / Mpc];  Om0 : Omega matter at z = 0;  Ob0 : Omega baryon at z = 0 (Omega CDM
        is Om0 - Ob0)
        """
        self.H0, self.Om0, self.Ob0 = float(H0), float(Om0), float(Ob0)
        self.Odm0 = self.Om0 - self.Ob0
        self.Tcmb0, self.Neff = 2.725, 3.05
        self.m_nu = np.array([0.0, 0.0, 0.06])               # eV
        self.Tnu0 = 0.7137658555036082 * self.Tcmb0
        H0_si = self.H0 * 1e3 / _MPC                          # 1 / s
        self.critical_density0 = 3 * H0_si ** 2 / (8 * np.pi * _G)    # kg / m^3
        self.Ogamma0 = 4 * _SIGMA_SB * self.Tcmb0 ** 4 / (_C ** 3 * self.critical_density0)
        self._nu_y = self.m_nu[self.m_nu > 0] / (_KB_EV * self.Tnu0)
        self._nmassless = int((self.m_nu == 0).sum())
        self.Onu0 = self.Ogamma0 * float(self.nu_relative_density(0.0))
        self.Ode0 = 1.0 - self.Om0 - self.Ogamma0 - self.Onu0
        self.Ok0 = 0.0
        self.hubble_distance = _C / 1e3 / self.H0             # Mpc

        # 21 cm specific quantities
        self._f21 = 1.420405751e9  # frequency of 21cm transition in Hz
        self._w21 = 0.211061140542  # 21cm wavelength in meters

    def nu_relative_density(self, z):
        """neutrino energy density relative to the photons' at redshift z (massless species contribute 1 each)"""
        z = np.asarray(z, dtype=np.float64)
        y = self._nu_y / (1.0 + z[..., None])
        massive = ((1.0 + (0.3173 * y) ** 1.83) ** (1.0 / 1.83)).sum(axis=-1)
        return 0.22710731766 * (self.Neff / 3.0) * (self._nmassless + massive)

    def efunc(self, z):
        """E(z) = H(z) / H0"""
        z = np.asarray(z, dtype=np.float64)
        zp1 = 1.0 + z
        return np.sqrt(self.Om0 * zp1 ** 3 + self.Ogamma0 * (1.0 + self.nu_relative_density(z)) * zp1 ** 4 + self.Ode0)

    def H(self, z):
        """Hubble parameter at redshift z [km / s / Mpc]"""
        return self.H0 * self.efunc(z)

    def comoving_distance(self, z):
        """
        Line-of-sight comoving distance [Mpc] to redshift z (scalar or array), a `Distance` (ndarray with `.value`):
            D = (c / H0) int_0^z dz' / E(z') = (c / H0) int_0^ln(1 + z) e^x / E(e^x - 1) dx
        by ONE Gauss-Legendre rule of order 64 in x = ln(1 + z), float64.  The integrand is analytic in a strip of half
        width pi / 3 around the real x axis (the nearest zero of E^2 is where matter and Lambda cancel), so the rule
        converges geometrically: for 0 <= z <= 30 (21 cm frequencies above 46 MHz) its error is below 1e-13 relative
        (measured: below 1e-15 against composite rules of two orders, tests/test_lcone_host.py), i.e. rounding level.
        """
        z = np.asarray(z, dtype=np.float64)
        half = 0.5 * np.log1p(z)[..., None]
        x = half * (_GL_X + 1.0)
        f = np.exp(x) / self.efunc(np.expm1(x))
        d = self.hubble_distance * (half[..., 0] * (f * _GL_W).sum(axis=-1))
        return np.asarray(d, dtype=np.float64).view(Distance)

    def comoving_transverse_distance(self, z):
        """the same as comoving_distance: the model is flat"""
        return self.comoving_distance(z)

    def f2z(self, freq):
        """frequency [Hz] of the 21 cm line to redshift"""
        return self._f21 / freq - 1

    def z2f(self, z):
        """redshift to frequency [Hz] of the 21 cm line"""
        return self._f21 / (z + 1)

    def f2r(self, f):
        """frequency [Hz] to line-of-sight comoving distance [Mpc]"""
        return self.comoving_distance(self.f2z(f)).value

    def r2f(self, r, rtol=1e-12, maxiter=200):
        """
        Line-of-sight comoving distance [Mpc] to frequency [Hz]: the root z of comoving_distance(z) = r inside a bracket
        [lo, hi] (hi doubled from 1 until it encloses r), by Newton steps with dD/dz = c / (H0 E) that fall back to
        bisection whenever a step leaves the bracket; converged when |D(z) - r| <= rtol r.  Scalar in, scalar out; array
        in, array out.
        """
        scalar = np.ndim(r) == 0
        r = np.atleast_1d(np.asarray(r, dtype=np.float64))
        if (r < 0).any() or not np.isfinite(r).all():
            raise ValueError('r2f: distances must be finite and non-negative')
        lo, hi = np.zeros_like(r), np.ones_like(r)
        for _ in range(64):
            short = np.asarray(self.comoving_distance(hi)) < r
            if not short.any():
                break
            lo[short] = hi[short]
            hi[short] *= 2.0
        else:
            raise ValueError('r2f: a distance lies beyond the horizon of this model')
        z = np.where(r == 0, 0.0, 0.5 * (lo + hi))
        for _ in range(maxiter):
            d = np.asarray(self.comoving_distance(z)) - r
            done = np.abs(d) <= rtol * r
            if done.all():
                break
            lo = np.where(d < 0, z, lo)
            hi = np.where(d >= 0, z, hi)
            step = z - d * self.efunc(z) / self.hubble_distance
            inside = (step > lo) & (step < hi)
            z = np.where(done, z, np.where(inside, step, 0.5 * (lo + hi)))
        else:
            raise RuntimeError('r2f: no convergence in %d iterations' % maxiter)
        f = self.z2f(z)
        return float(f[0]) if scalar else f

    def dRperp_dtheta(self, z):
        """angular size [rad] to transverse comoving distance [Mpc] at redshift z: [Mpc / rad]"""
        return self.comoving_transverse_distance(z).value

    def dRpara_df(self, z):
        """frequency bandwidth to radial comoving distance at redshift z: [Mpc / Hz]"""
        return (1 + z)**2.0 / self.H(z) * (_C / 1e3) / self._f21

    def X2Y(self, z):
        """rad^2 Hz to Mpc^3 at redshift z: [Mpc^3 / (rad^2 Hz)]"""
        return self.dRperp_dtheta(z)**2 * self.dRpara_df(z)

    def bl_to_kperp(self, z):
        """baseline length [m] to transverse wavevector k_perp: [Mpc^-1 / m] (Parsons 2012, Pober 2014, Kohn 2018)"""
        return 2 * np.pi / (self.dRperp_dtheta(z) * (_C / self.z2f(z)))

    def tau_to_kpara(self, z):
        """delay [s] to line-of-sight wavevector k_parallel: [Mpc^-1 / s]"""
        return 2 * np.pi / self.dRpara_df(z)


def gauss1d(x, scale=1.0, loc=0.0):
    """
    1D Gaussian window at the points x ((Nsamples,) or (Nfeatures, Nsamples)) of standard deviation `scale` and mean `loc`,
    normalised to sum(win) = 1 along the samples
    """
    w = np.atleast_2d(np.exp(-0.5 * (x - loc)**2 / scale**2))
    w /= w.sum(axis=1, keepdims=True)
    if w.size == 1:
        w = w[0, 0]

    return w


# ------------------------------------------------------------------------------------------------- lightcone sampling
RINTERP = {'nearest': 1, 'linear': 2, 'quadratic': 3}


def radial_stencil(sim_r, r, rinterp='nearest'):
    """
    (cube_idx (Nr, 3) int32, weight (Nr, 3) float64, S) of the radial interpolation of cubes at distances sim_r to the
    distances r, numpy float64 on the host.  The cubes are the S nearest to r in |r - sim_r| (ties: the lower index), in
    index order -- the reference's choice, not necessarily a bracket, so for an r outside sim_r the weights may be negative
    or exceed 1.  'nearest': S = 1, weight 1.  'linear': S = 2, t = (r - r1) / (r2 - r1), weights (1 - t, t).  'quadratic':
    S = 3, the Lagrange parabola through the three cubes.  Unused columns hold cube 0 and weight 0.
    """
    if rinterp not in RINTERP:
        raise ValueError("rinterp must be 'nearest', 'linear' or 'quadratic' (got %r)" % (rinterp,))
    S = RINTERP[rinterp]
    sim_r = np.asarray(sim_r, dtype=np.float64).reshape(-1)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    if sim_r.size < S:
        raise ValueError("rinterp=%r needs %d cubes, sim_r has %d" % (rinterp, S, sim_r.size))
    idx = np.zeros((r.size, 3), dtype=np.int32)
    wgt = np.zeros((r.size, 3), dtype=np.float64)
    for i, ri in enumerate(r):
        s = np.sort(np.argsort(np.abs(ri - sim_r), kind='stable')[:S])
        idx[i, :S] = s
        x = sim_r[s]
        if S == 1:
            wgt[i, 0] = 1.0
        elif S == 2:
            t = (ri - x[0]) / (x[1] - x[0])
            wgt[i, :2] = 1.0 - t, t
        else:
            wgt[i, 0] = (ri - x[1]) * (ri - x[2]) / ((x[0] - x[1]) * (x[0] - x[2]))
            wgt[i, 1] = (ri - x[0]) * (ri - x[2]) / ((x[1] - x[0]) * (x[1] - x[2]))
            wgt[i, 2] = (ri - x[0]) * (ri - x[1]) / ((x[2] - x[0]) * (x[2] - x[1]))
    return idx, wgt, S


def unit_vectors(angs):
    """(3, Npix) float64 unit vectors of (theta, phi) co-latitude and eastward longitude [rad], as the reference forms them"""
    theta, phi = np.asarray(angs.detach().cpu() if torch.is_tensor(angs) else angs, dtype=np.float64)
    sintheta = np.sin(theta)
    return np.stack([sintheta * np.cos(phi), sintheta * np.sin(phi), np.cos(theta)])


def _roll3(roll):
    if roll is None:
        return (0, 0, 0)
    if isinstance(roll, (int, np.integer)):
        return (int(roll),) * 3
    roll = tuple(int(x) for x in roll)
    if len(roll) != 3:
        raise ValueError('roll must be an int or (x, y, z)')
    return roll


def cube2lcone(sims, sim_r, r, sim_res, angs=None, rinterp='nearest',
               interp='nearest', cosmo=None, roll=None):
    """
    Project simulation cubes onto a lightcone, in one kernel launch for all radii and pixels.

    Parameters
    ----------
    sims : ndarray, tensor or str
        Temperature simulation cubes of shape (Nsim_r, Nx, Ny, Nz) or one cube (Nx, Ny, Nz), float32 or float64 (anything
        else raises TypeError), or the path of a .npy file of them.  A numpy array gives a numpy array (through the GPU), a
        tensor on the GPU a tensor on that device; the dtype follows the cubes.
    sim_r : ndarray
        Comoving distances of the cubes [Mpc]
    r : ndarray or float
        Comoving radial distances to interpolate to [Mpc]
    sim_res : float
        Voxel size [cMpc]
    angs : ndarray, optional
        (theta, phi) co-latitude and eastward longitude of shape (2, Npix) [rad].  None: the cube's own (x, y) grid, only
        z is sampled ("plane" mode, output (Nr, Nx, Ny)).
    rinterp : str, optional
        Radial interpolation between cubes: 'nearest', 'linear', 'quadratic' (see radial_stencil)
    interp : str, optional
        Spatial interpolation: 'nearest' (np.around's voxel) or 'linear' (trilinear)
    cosmo : unused, as in the reference
    roll : int or tuple, optional
        Roll of the cubes along x, y, z before sampling (np.roll's meaning), folded into the index arithmetic

    Returns
    -------
    (Nr, Npix) or (Nr, Nx, Ny)

    Deviations from the reference, deliberate:
      1. 'quadratic' is the parabola through its three cubes.  The reference's branch assigns sim1 = sims[s2] and uses
         sim3 - sim1 where its own derivation needs sim3 - sim2, so it is not; its output is not reproduced.
      2. a 3-D `sims` is ONE cube used for every r, and rinterp must then be 'nearest' (the reference would index the
         cube's x axis with the cube number).
      3. rinterp 'linear' / 'quadratic' with fewer than 2 / 3 cubes raises ValueError.
    Positions are float64 whatever the cube dtype; the sum over cubes and corners runs in the cube dtype in the fixed
    order of csrc/lcone.hip, so the same input gives the same bits.  No CPU path.
    """
    if isinstance(sims, str):
        sims = np.load(sims)
    if interp not in ops.LCONE_INTERP:
        raise ValueError("interp must be 'nearest' or 'linear' (got %r)" % (interp,))
    if rinterp not in RINTERP:
        raise ValueError("rinterp must be 'nearest', 'linear' or 'quadratic' (got %r)" % (rinterp,))
    as_numpy = not torch.is_tensor(sims)
    cubes = torch.as_tensor(np.asarray(sims)) if as_numpy else sims
    if cubes.dtype not in (torch.float32, torch.float64):
        raise TypeError('cube2lcone serves float32 and float64 cubes (got %s)' % cubes.dtype)
    if cubes.ndim == 3:
        if rinterp != 'nearest':
            raise ValueError("a single 3-D cube has no radial axis to interpolate: rinterp must be 'nearest'")
        cubes = cubes[None]
        sim_r = np.zeros(1)
    elif cubes.ndim != 4:
        raise ValueError('sims must be (Nsim_r, Nx, Ny, Nz) or (Nx, Ny, Nz)')
    sim_r = np.asarray(sim_r.detach().cpu() if torch.is_tensor(sim_r) else sim_r, dtype=np.float64).reshape(-1)
    if sim_r.size != cubes.shape[0]:
        raise ValueError('sim_r has %d entries for %d cubes' % (sim_r.size, cubes.shape[0]))
    r = np.atleast_1d(np.asarray(r.detach().cpu() if torch.is_tensor(r) else r, dtype=np.float64)).reshape(-1)
    idx, wgt, S = radial_stencil(sim_r, r, rinterp)
    vec = None if angs is None else unit_vectors(angs)
    roll = _roll3(roll)
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("bayeslim_amd ops need a GPU (none found); there is no CPU implementation")
        cubes = cubes.cuda()
    out = ops.lcone_sample(cubes, r, idx, wgt, S, sim_res, vec=vec, roll=roll, interp=interp)
    return out.cpu().numpy() if as_numpy else out


def cube2map(cube, dc, sim_res, angs=None, roll=None, interp='nearest'):
    """
    Tile a simulation cube (Nx, Ny, Nz), aligned as (x, y, z) with z the line of sight, periodically and extract a map at
    the comoving distance dc [Mpc] (after P. Kittiwisit's cosmotile): onto `angs` (theta, phi) of shape (2, Npix), or, with
    angs None, onto the cube's own (x, y) grid with only z interpolated.  sim_res: voxel size [cMpc]; roll, interp: see
    cube2lcone, of which this is the row of one cube at one distance.
    """
    if getattr(cube, 'ndim', None) != 3:
        raise ValueError('cube must be (Nx, Ny, Nz)')
    return cube2lcone(cube, None, [float(dc)], sim_res, angs=angs, rinterp='nearest', interp=interp, roll=roll)[0]
