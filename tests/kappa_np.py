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


def centred_longdouble(maps):
    """(m_p - mean m_p, mean m_p) in np.longdouble (64-bit mantissa on x86): the reference side of the derived bound."""
    m = np.asarray(maps).astype(np.longdouble)
    mu = m.reshape(len(m), -1).mean(axis=1)
    return m - mu[:, None, None], mu


def mean_depth(npix):
    """D: the number of f64 roundings on the path of one pixel to a plane mean in slicer_lensing.hip -- the 4-pixel sum
    of a lane (2), 6 butterfly levels, 2 levels over the 4 waves, ceil(nblocks / 256) sequential partials per thread,
    8 tree levels, one division; nblocks = ceil(npix^2 / 1024)."""
    nblocks = -(-npix * npix // 1024)
    return 18 + -(-nblocks // 256)


def kappa_bound(ref, maps, mu, c_s, n_batches):
    """The derived bound of the device kappa of one source against the exact value `ref` (np.longdouble), per pixel:
        2^-24 |ref| (1 + 2^-20)  +  K 2^-53 sum_p |c_sp| (|m_p| + |mu_p|),   K = P + n_batches + D + 8.
    First term: the one rounding of (A - off) to f32 (half an ulp of a value within 2^-20 of ref).  Second term: the f64
    roundings -- at most P products and P additions folded into sum_p (P + n_batches additions into A over the
    batches), the D roundings behind every mean, and a handful for the sum over the means and the final subtraction.
    Nothing in it is measured.  If long double is not wider than f64, the reference's own (P + 2) 2^-53 is added."""
    P = len(maps)
    K = P + n_batches + mean_depth(maps.shape[-1]) + 8
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        K += P + 2
    c = np.abs(np.asarray(c_s, np.float64)).astype(np.longdouble)
    mag = np.zeros(maps.shape[1:], np.longdouble)
    for p in range(P):
        if c[p] != 0:
            mag += c[p] * (np.abs(maps[p]).astype(np.longdouble) + abs(mu[p]))
    L = np.longdouble
    return L(2.0 ** -24) * np.abs(ref) * (1 + L(2.0 ** -20)) + K * L(2.0 ** -53) * mag


def kappa_longdouble(centred, c_s):
    """kappa of one source from centred_longdouble's maps, in np.longdouble."""
    ref = np.zeros(centred.shape[1:], np.longdouble)
    for p, c in enumerate(np.asarray(c_s, np.float64)):
        if c != 0:
            ref += np.longdouble(c) * centred[p]
    return ref


def worst_ratio(got, maps, coeff, n_batches):
    """max over sources and pixels of |got - ref| / bound (0 where both are 0); got [S, npix, npix] f32."""
    maps = np.asarray(maps)
    centred, mu = centred_longdouble(maps)
    worst = 0.0
    for s in range(len(coeff)):
        ref = kappa_longdouble(centred, coeff[s])
        bound = kappa_bound(ref, maps, mu, coeff[s], n_batches)
        err = np.abs(got[s].astype(np.longdouble) - ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)  # err > 0 over a zero bound: inf
        worst = max(worst, float(ratio.max()))
    return worst


def mean_bound(maps):
    """(D + 2) 2^-53 mean|m_p| per plane: the summation tree of mean_depth, the division and the reference."""
    m = np.asarray(maps)
    return (mean_depth(m.shape[-1]) + 2) * 2.0 ** -53 * np.abs(m).astype(np.float64).reshape(len(m), -1).mean(axis=1)


def planes_and_weights(npix, n_src):
    """The planes, weights and batch sizes of tests/test_gpu_kappa.py::test_kappa_matches_numpy (shared with the
    host-only test of the bound)."""
    rng = np.random.default_rng(npix * 100 + n_src)
    batches = [1, 4, 8] if npix != 4096 else [4]
    P = sum(batches)
    maps = (rng.gamma(0.5, 2.0, (P, npix, npix)) * 3.0).astype(np.float32)
    coeff = rng.uniform(1e-5, 1e-3, (n_src, P))
    coeff[:, rng.random(P) < 0.25] = 0.0          # planes behind some sources
    if n_src > 1:
        coeff[1] = 0.0                            # a source with no plane at all
    return maps, coeff, batches


def emulate(maps, coeff, batches, acc):
    """The arithmetic of slicer_kappa_add / _finalize with accumulators of type `acc`: per batch t = sum_p c m in plane
    order, A += t, off += sum_p c mean_p; result (float)(A - off).  acc = np.float64 is the contract; np.float32 is the
    wrong kernel the bound has to catch."""
    S, (P, n, _) = len(coeff), maps.shape
    A = np.zeros((S, n, n), acc)
    off = np.zeros(S, acc)
    p0 = 0
    for b in batches:
        for s in range(S):
            t = np.zeros((n, n), acc)
            o = acc(0)
            for p in range(p0, p0 + b):
                t += acc(coeff[s, p]) * maps[p].astype(acc)
                o += acc(coeff[s, p]) * acc(maps[p].astype(np.float64).mean())
            A[s] += t
            off[s] += o
        p0 += b
    return (A - off[:, None, None]).astype(np.float32)
