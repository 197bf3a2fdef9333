"""Restatement of the moments-over-a-halving-pyramid contract (include/slicer_amd.h) in numpy:
halving in f32 in the stated order, moments in long double, the depth formula, the bounds, and emulate(), which follows
the device's summation order with a chosen accumulator type."""
import numpy as np

LD = np.longdouble
ORDERS = tuple(range(2, 9))
U = 2.0 ** -53
THREADS, ITEMS, WAVE = 256, 8, 64
GROUP = THREADS * ITEMS


def halve(x, mode="mean"):
    """One level down: ((x[2i,2j] + x[2i+1,2j]) + x[2i,2j+1]) + x[2i+1,2j+1] in f32, times 0.25f in mode "mean"."""
    x = np.asarray(x, np.float32)
    h = x.shape[0] // 2
    a, b, c, d = (x[r:2 * h:2, s:2 * h:2] for r, s in ((0, 0), (1, 0), (0, 1), (1, 1)))
    y = ((a + b).astype(np.float32) + c).astype(np.float32) + d
    y = y.astype(np.float32)
    return (np.float32(0.25) * y).astype(np.float32) if mode == "mean" else y


def pyramid(x, levels, mode="mean"):
    out = [np.asarray(x, np.float32)]
    for _ in range(levels):
        out.append(halve(out[-1], mode))
    return out


def mean_ld(x):
    """(mean, mean|x|) in long double."""
    v = np.asarray(x, np.float32).astype(LD).ravel()
    return v.sum() / LD(v.size), np.abs(v).sum() / LD(v.size)


def sums_ld(x, c):
    """S_k and A_k = sum |x - c|^k, k = 2 ... 8, in long double about the f64 centre c."""
    d = np.asarray(x, np.float32).astype(LD).ravel() - LD(np.float64(c))
    a = np.abs(d)
    S, A, p, q = [], [], d, a
    for _ in ORDERS:
        p, q = p * d, q * a
        S.append(p.sum())
        A.append(q.sum())
    return np.array(S, LD), np.array(A, LD)


def _cdiv(a, b):
    return -(-a // b)


def geometry(n):
    h = n // 2
    Q = (h + 1) // 2
    T = h * Q
    Tall = T + (_cdiv(2 * n - 1, 8) if n % 2 else 0)
    Ty = n * ((n + 1) // 2)
    return {"n": n, "h": h, "Q": Q, "T": T, "Tall": Tall, "G": _cdiv(Tall, GROUP), "Ty": Ty, "Gy": _cdiv(Ty, GROUP)}


def depth(n):
    """D(n): f64 additions on the longest path of either tree, counted from the kernels: a thread's own additions
    (8 or 2 per item, at most 8 items), butterfly 6, waves 3, then partials ceil(G / 256), butterfly 6, waves 3."""
    g = geometry(n)
    a = 8 * min(ITEMS, _cdiv(g["Tall"], THREADS)) + 18 + _cdiv(g["G"], THREADS)
    b = 2 * min(ITEMS, _cdiv(g["Ty"], THREADS)) + 18 + _cdiv(g["Gy"], THREADS)
    return max(a, b)


def sum_bounds(A, n):
    """(2k - 1 + D) u (1 + 2^-20) A_k for k = 2 ... 8."""
    D = depth(n)
    return np.array([(2 * k - 1 + D) * U * (1 + 2.0 ** -20) for k in ORDERS], LD) * A


def mean_bound(mean_abs, n):
    return (depth(n) + 2) * U * mean_abs


# ---- the device's order -------------------------------------------------------------------------------

def _workgroup_sum(acc):
    """acc [..., 256] per-thread values -> [...]: butterfly in every wave, then the waves in order."""
    lanes = np.arange(WAVE)
    w = acc.reshape(acc.shape[:-1] + (THREADS // WAVE, WAVE))
    off = WAVE // 2
    while off >= 1:
        w = w + w[..., lanes ^ off]
        off //= 2
    w = w[..., 0]
    r = w[..., 0]
    for k in range(1, THREADS // WAVE):
        r = r + w[..., k]
    return r


def _tree(vals, ok, dtype):
    """vals, ok [T, S]: item t's S values in order (ok: which of them exist).  Workgroup b takes items b * 2048 ...,
    thread tid item b * 2048 + j * 256 + tid for j = 0 ... 7; then the partials: thread t takes t, t + 256, ..."""
    T, S = vals.shape
    G = _cdiv(T, GROUP)
    v = np.zeros((G * GROUP, S), dtype)
    m = np.zeros((G * GROUP, S), bool)
    v[:T], m[:T] = vals, ok
    v = v.reshape(G, ITEMS, THREADS, S).transpose(0, 2, 1, 3).reshape(G, THREADS, ITEMS * S)
    m = m.reshape(G, ITEMS, THREADS, S).transpose(0, 2, 1, 3).reshape(G, THREADS, ITEMS * S)
    acc = np.zeros((G, THREADS), dtype)
    for e in range(ITEMS * S):
        acc = np.where(m[..., e], acc + v[..., e], acc)
    part = _workgroup_sum(acc)
    R = _cdiv(G, THREADS)
    p = np.zeros(R * THREADS, dtype)
    p[:G] = part
    pm = np.arange(R * THREADS).reshape(R, THREADS) < G
    p = p.reshape(R, THREADS)
    acc = np.zeros(THREADS, dtype)
    for r in range(R):
        acc = np.where(pm[r], acc + p[r], acc)
    return _workgroup_sum(acc)


def item_pixels(n):
    """(flat pixel index [Tall, 8], exists [Tall, 8]) of the moment pass over an n x n level."""
    g = geometry(n)
    h, Q, T, Tall = g["h"], g["Q"], g["T"], g["Tall"]
    idx = np.zeros((Tall, 8), np.int64)
    ok = np.zeros((Tall, 8), bool)
    if T:
        t = np.arange(T)
        i, q = t // Q, t % Q
        for e in range(4):
            col = 4 * q + e
            inside = col < 2 * h
            idx[:T, e] = np.where(inside, 2 * i * n + col, 0)
            idx[:T, 4 + e] = np.where(inside, (2 * i + 1) * n + col, 0)
            ok[:T, e] = ok[:T, 4 + e] = inside
    if n % 2:
        p = 8 * np.arange(Tall - T)[:, None] + np.arange(8)[None, :]
        exists = p < 2 * n - 1
        at = np.where(p < n, (n - 1) * n + p, (p - n) * n + (n - 1))
        idx[T:] = np.where(exists, at, 0)
        ok[T:] = exists
    return idx, ok


def emulate_mean(x, dtype=np.float64):
    """The mean in the order of k_moments_sum / of the halving pass that writes x: items of two adjacent pixels."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    Qm = (n + 1) // 2
    t = np.arange(n * Qm)
    i, q = t // Qm, t % Qm
    cols = np.stack([2 * q, 2 * q + 1], 1)
    ok = cols < n
    vals = x.ravel()[np.where(ok, i[:, None] * n + cols, 0)].astype(dtype)
    return _tree(vals, ok, dtype) / dtype(n * n)


def emulate(x, c, acc_dtype=np.float64):
    """(S_2 ... S_8, mean) of one level as the device sums them, every operation in acc_dtype."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    idx, ok = item_pixels(n)
    d = x.ravel()[idx].astype(acc_dtype) - acc_dtype(c)
    p = d * d
    sums = [_tree(p, ok, acc_dtype)]
    for _ in ORDERS[1:]:
        p = p * d
        sums.append(_tree(p, ok, acc_dtype))
    return np.array(sums, acc_dtype), emulate_mean(x, acc_dtype)
