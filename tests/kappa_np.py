"""Independent numpy / scipy restatement of the Born convergence contract: quad for the
distances, brentq for z(chi), solve_ivp for the growth factor.  Shared by the kappa tests."""
import numpy as np
from scipy.integrate import quad, solve_ivp
from scipy.optimize import brentq

C_LIGHT = 299792458.0
G_NEWTON = 6.67430e-11
M_SUN = 1.988409870698051e30
MPC = 3.0856775814913673e22
C2_OVER_G = C_LIGHT ** 2 / G_NEWTON * MPC / M_SUN / 1e10  # 1e10 Msun / Mpc
DH = 2997.92458  # Mpc/h


class Flat:
    def __init__(self, om, w0=-1.0, wa=0.0):
        self.om, self.ol, self.w0, self.wa = om, 1.0 - om, w0, wa

    def E(self, z):
        a1 = 1.0 + z
        de = self.ol * a1 ** (3 * (1 + self.w0 + self.wa)) * np.exp(-3 * self.wa * z / a1)
        return np.sqrt(self.om * a1 ** 3 + de)

    def chi(self, z):
        if z <= 0:
            return 0.0
        return DH * quad(lambda x: 1.0 / self.E(x), 0.0, z, epsabs=0, epsrel=1e-13, limit=200)[0]

    def z_of_chi(self, d):
        if d <= 0:
            return 0.0
        return brentq(lambda z: self.chi(z) - d, 0.0, 20.0, xtol=1e-15, rtol=1e-15, maxiter=500)

    def growth(self, zs):
        """D+ at the redshifts zs (unnormalised), from D'' + (2 + dlnE/dlna) D' = 3/2 Om(a) D in ln a."""
        def rhs(x, y):
            a = np.exp(x)
            z = 1 / a - 1
            e2 = self.E(z) ** 2
            de = self.ol * a ** (-3 * (1 + self.w0 + self.wa)) * np.exp(-3 * self.wa * (1 - a))
            dlne = 0.5 * (-3 * self.om * a ** -3 + de * (-3 * (1 + self.w0 + self.wa) + 3 * self.wa * a)) / e2
            return [y[1], -(2 + dlne) * y[1] + 1.5 * self.om * a ** -3 / e2 * y[0]]
        x0 = np.log(1e-5)
        xs = -np.log1p(np.atleast_1d(np.asarray(zs, np.float64)))
        grid, where = np.unique(xs, return_inverse=True)
        sol = solve_ivp(rhs, (x0, grid[-1]), [np.exp(x0), np.exp(x0)], method="DOP853", rtol=1e-13, atol=1e-20,
                        t_eval=grid)
        return sol.y[0][where]


def weights(om, w0, fov_deg, npix, ld, ld2, zsnap, zs=None, growth=True):
    """-> (c[S, P], zlo, zup, zl, chil)."""
    cos = Flat(om, w0)
    P = len(ld)
    zlo = np.array([cos.z_of_chi(d) for d in ld])
    zup = np.array([cos.z_of_chi(d) for d in ld2])
    zl = np.empty(P)
    for p in range(P):
        num = quad(lambda z: z * cos.chi(z), zlo[p], zup[p], epsabs=0, epsrel=1e-13)[0]
        den = quad(lambda z: cos.chi(z), zlo[p], zup[p], epsabs=0, epsrel=1e-13)[0]
        zl[p] = num / den
    chil = np.array([cos.chi(z) for z in zl])
    g = cos.growth(zl) / cos.growth(zsnap) if growth else np.ones(P)
    area = (2 * chil * np.tan(fov_deg * np.pi / 360)) ** 2 / npix ** 2
    zs = zup if zs is None else np.asarray(zs, np.float64)
    c = np.zeros((len(zs), P))
    for s, z in enumerate(zs):
        chis = cos.chi(z)
        for p in range(P):
            if zup[p] <= z + 1e-4:
                eff = (chil[p] / (1 + zl[p])) * ((chis - chil[p]) / (1 + z)) / (chis / (1 + z))
                c[s, p] = 4 * np.pi / C2_OVER_G * eff * g[p] * (1 + zl[p]) ** 2 / area[p]
    return c, zlo, zup, zl, chil


def kappa(maps, c):
    """kappa_s = sum_p c[s, p] (m_p - mean m_p) in f64."""
    m = np.asarray(maps, np.float64)
    mu = m.reshape(len(m), -1).mean(axis=1)
    return np.einsum("sp,pij->sij", c, m - mu[:, None, None])
