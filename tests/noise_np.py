"""numpy restatement of slicer_noise_* (DESIGN.md S8 row N13).  It imports nothing from the library.

Philox4x32-10 on uint64 arrays, Box-Muller in long double from the exact words, the output formula, and the bound:
    |out - ref| <= 2^-24 |ref| (1 + 2^-20) + K 2^-53 sigma R,   K = 8 (DESIGN.md counts it),
with the condition that out differs from RN32(ref) in at most 1e-4 of a map's pixels.  Two emulations of an evaluation
(f64 as the device does it, f32 as it must not) serve the test that the bound tells them apart."""
import numpy as np

LD = np.longdouble
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
K = 8
SHARE = 1e-4
PI_LD = LD("3.14159265358979323846264338327950288")


def philox(c0, c1, c2, c3, k0, k1):
    """Ten rounds on uint64 arrays holding 32-bit values; -> [..., 4] uint32."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(a, np.uint64) & MASK for a in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # below 2^64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def words(seed, stream, realisation, block):
    """The words of blocks `block` (u64): counter (lo b, hi b, realisation, stream), key (lo seed, hi seed)."""
    b, seed = np.asarray(block, np.uint64), np.asarray(seed, np.uint64)
    return philox(b & MASK, b >> S32, realisation, stream, seed & MASK, seed >> S32)


def _sincospi_ld(t):
    """(sinpi t, cospi t) in long double for t = 2 u in (0, 2): reduced exactly to |r| <= 1/4 about a multiple of 1/2."""
    q = np.floor(2 * t + LD(0.5))
    r = t - q / 2  # exact
    a = PI_LD * r
    s, c = np.sin(a), np.cos(a)
    q = q.astype(np.int64) % 4
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def normals(w):
    """(z, R): [..., 4] long double normals of [..., 4] words and each one's own R."""
    w = np.asarray(w, np.uint32).astype(LD)
    u = (w + LD(0.5)) * LD(2.0) ** -32
    ra, rb = np.sqrt(-2 * np.log(u[..., 0])), np.sqrt(-2 * np.log(u[..., 2]))
    sa, ca = _sincospi_ld(2 * u[..., 1])
    sb, cb = _sincospi_ld(2 * u[..., 3])
    return np.stack([ra * ca, ra * sa, rb * cb, rb * sb], -1), np.stack([ra, ra, rb, rb], -1)


def field(seed, stream, realisation, first_pixel, count):
    """(z, R) of the flat pixels first_pixel ... first_pixel + count - 1 (first_pixel a multiple of 4), long double [count]."""
    assert first_pixel % 4 == 0
    nb = (count + 3) // 4
    blocks = (np.uint64(first_pixel // 4) + np.arange(nb, dtype=np.uint64))
    z, R = normals(words(seed, stream, realisation, blocks))
    return z.reshape(-1)[:count], R.reshape(-1)[:count]


def reference(x, sigma, seed, stream=0, realisation=0, first_pixel=0, count=None):
    """(ref, R) in long double: x + sigma z of the flat f32 array x (None: the noise alone, `count` values)."""
    if x is not None:
        x = np.asarray(x, np.float32).ravel()
        count = x.size
    z, R = field(seed, stream, realisation, first_pixel, count)
    ref = LD(sigma) * z
    if x is not None:
        with np.errstate(invalid="ignore"):
            ref = x.astype(LD) + ref
    return ref, R


def check(out, ref, R, sigma, k=K):
    """-> (inside the bound everywhere, share of the pixels that differ from RN32(ref), worst error in units of
    2^-53 sigma R after the f32 rounding's allowance; negative: inside that allowance alone).  Pixels whose reference
    is not finite must be equal as values."""
    out = np.asarray(out, np.float32).ravel()
    fin = np.isfinite(ref)
    same_special = bool(np.all((out[~fin] == ref[~fin].astype(np.float32)) | (np.isnan(out[~fin]) & np.isnan(ref[~fin]))))
    o, r, rr = out[fin].astype(LD), ref[fin], R[fin]
    err = np.abs(o - r)
    allow32 = LD(2.0) ** -24 * np.abs(r) * (1 + LD(2.0) ** -20)
    unit = LD(2.0) ** -53 * LD(sigma) * rr
    ok = bool(np.all(err <= allow32 + k * unit)) and same_special
    with np.errstate(divide="ignore", invalid="ignore"):
        over = np.where(unit > 0, (err - allow32) / unit, 0)
    worst = float(over.max()) if over.size else 0.0
    share = float(np.count_nonzero(out[fin] != r.astype(np.float32))) / max(out.size, 1)
    return ok, share, worst


def _sincospi(t, dtype):
    """The device's form in `dtype`: exact reduction, then sin and cos of pi r."""
    q = np.floor(2 * t + dtype(0.5))
    r = (t - q / dtype(2)).astype(dtype)
    a = (dtype(np.pi) * r).astype(dtype)
    s, c = np.sin(a), np.cos(a)
    q = q.astype(np.int64) % 4
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def emulate(x, sigma, seed, stream, realisation, count, dtype):
    """out as an evaluation in `dtype` (np.float64: what the device does; np.float32: u, log, sqrt, sincos and the
    products all in f32) would give it."""
    nb = (count + 3) // 4
    w = words(seed, stream, realisation, np.arange(nb, dtype=np.uint64)).astype(np.float64)
    u = ((w + 0.5) * 2.0 ** -32).astype(dtype)
    if dtype is np.float32:
        u = np.minimum(u, np.float32(1) - np.float32(2.0 ** -24))  # (an f32 u rounds to 1 for the largest words)
    t = ((w + 0.5) * 2.0 ** -31).astype(dtype)
    ra, rb = np.sqrt(dtype(-2) * np.log(u[:, 0])), np.sqrt(dtype(-2) * np.log(u[:, 2]))
    sa, ca = _sincospi(t[:, 1], dtype)
    sb, cb = _sincospi(t[:, 3], dtype)
    z = np.stack([ra * ca, ra * sa, rb * cb, rb * sb], -1).astype(dtype).reshape(-1)[:count]
    n = (dtype(sigma) * z).astype(dtype)
    if x is None:
        return n.astype(np.float32)
    return (np.asarray(x, np.float32).ravel().astype(np.float64) + n.astype(np.float64)).astype(np.float32)
