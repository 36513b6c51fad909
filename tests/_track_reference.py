"""Numpy restatement of include/fdf.h's pyramidal Lucas-Kanade rules: the sample, the level maps
and the sums in Python integers / int64, the 2 x 2 solve in float64 one operation at a time
(numpy never fuses a multiply with an add).  A point's window is vectorised, the points are not.
Nothing here calls the library; the tests compare the library with this, bit for bit."""
import numpy as np

ONE = 2048
STEP_LIMIT = 1 << 20
SKIPPED, TRACKED, LOST_EIGEN, LOST_FRAME, LOST_STEP = 0, 1, 2, 3, 4
NO_ERR = 0xFFFFFFFF
MATCH_NONE = 0xFFFFFFFF
COORDS_U32, COORDS_Q11 = 0, 2


def map_pos(x, len0, lenl):
    """A level-0 Q11 position on an axis of length ``len0`` at a level of length ``lenl``."""
    x, len0, lenl = int(x), int(len0), int(lenl)
    v = ((x + 1024) * lenl * 2 + len0) // (2 * len0) - 1024
    return min(max(v, 0), (lenl - 1) * ONE)


def map_disp(d, len_from, len_to):
    """A Q11 displacement carried between levels (floor division, for negative ``d`` too)."""
    d, len_from, len_to = int(d), int(len_from), int(len_to)
    return (2 * d * len_to + len_from) // (2 * len_from)


def sample(img, X, Y):
    """S at the Q11 positions (X, Y) (int64 arrays of one shape): 0..8160, taps clamped."""
    img = np.asarray(img)
    h, w = img.shape
    src = img.astype(np.int64)
    X = np.asarray(X, dtype=np.int64)
    Y = np.asarray(Y, dtype=np.int64)
    ix, qx = X >> 11, X & 2047
    iy, qy = Y >> 11, Y & 2047
    total = np.zeros(np.broadcast(X, Y).shape, dtype=np.int64)
    for b, wy in ((0, ONE - qy), (1, qy)):
        for a, wx in ((0, ONE - qx), (1, qx)):
            total = total + wy * wx * src[np.clip(iy + b, 0, h - 1), np.clip(ix + a, 0, w - 1)]
    return (total + (1 << 16)) >> 17


def window(img, X, Y, half):
    """S on the (2 half + 1)^2 grid around (X, Y), [j + half, i + half] = S(X + 2048 i, Y + 2048 j)."""
    k = np.arange(-half, half + 1, dtype=np.int64) * ONE
    return sample(img, X + k[None, :], Y + k[:, None])


def scharr(P):
    """(Gx, Gy) of a patch with a one-pixel rim: the rim is dropped."""
    c = slice(1, -1)
    gx = (3 * (P[:-2, 2:] - P[:-2, :-2]) + 10 * (P[c, 2:] - P[c, :-2]) + 3 * (P[2:, 2:] - P[2:, :-2]))
    gy = (3 * (P[2:, :-2] - P[:-2, :-2]) + 10 * (P[2:, c] - P[:-2, c]) + 3 * (P[2:, 2:] - P[:-2, 2:]))
    return gx, gy


def tau_of(min_eig, radius):
    n = (2 * radius + 1) ** 2
    return np.multiply(np.multiply(np.float64(np.float32(min_eig)), np.float64(n)), 1048576.0)


def _inside(X, Y, w, h):
    return 0 <= X <= (w - 1) * ONE and 0 <= Y <= (h - 1) * ONE


def _round_step(v):
    """floor(v * 65536 + 0.5) as a Python int, or None unless |.| <= 2^20 (None for a NaN)."""
    with np.errstate(all="ignore"):
        f = np.floor(np.add(np.multiply(v, 65536.0), 0.5))
    if not (f >= -STEP_LIMIT and f <= STEP_LIMIT):
        return None
    return int(f)


def track_point(prev, nxt, X0, Y0, guess=None, radius=10, max_iters=30, eps=20, min_eig=1e-3,
                trace=None):
    """One point through the levels.  ``prev`` and ``nxt`` are lists of (H_l, W_l) uint8 arrays,
    level 0 first.  Returns (reason, Xn, Yn, err, iterations); Xn = Yn = -1 and err = NO_ERR unless
    reason == TRACKED.  ``trace`` (a list) receives a dict per visited level."""
    X0, Y0 = int(X0), int(Y0)
    r = int(radius)
    L = len(prev)
    h0, w0 = prev[0].shape
    lost = lambda reason, it: (reason, -1, -1, NO_ERR, it)
    if not _inside(X0, Y0, w0, h0):
        return lost(SKIPPED, 0)
    if guess is not None and not _inside(int(guess[0]), int(guess[1]), w0, h0):
        return lost(SKIPPED, 0)
    tau = tau_of(min_eig, r)
    hl, wl = prev[L - 1].shape
    Dx = Dy = 0
    if guess is not None:
        Dx = map_disp(int(guess[0]) - X0, w0, wl)
        Dy = map_disp(int(guess[1]) - Y0, h0, hl)
    iters = 0
    for l in range(L - 1, -1, -1):
        H, W = prev[l].shape
        if l < L - 1:
            hu, wu = prev[l + 1].shape
            Dx, Dy = map_disp(Dx, wu, W), map_disp(Dy, hu, H)
        Xp, Yp = map_pos(X0, w0, W), map_pos(Y0, h0, H)
        P = window(prev[l], Xp, Yp, r + 1)
        gx, gy = scharr(P)
        P = P[1:-1, 1:-1]
        A11, A12, A22 = int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
        a11, a12, a22 = np.float64(A11), np.float64(A12), np.float64(A22)
        p, q = np.subtract(a11, tau), np.subtract(a22, tau)
        usable = bool(np.add(p, q) > 0 and
                      np.subtract(np.multiply(p, q), np.multiply(a12, a12)) > 0)
        if trace is not None:
            trace.append({"level": l, "A": (A11, A12, A22), "usable": usable, "b": [], "pos": []})
        if not usable:
            if l == 0:
                return lost(LOST_EIGEN, iters)
            continue
        det = np.subtract(np.multiply(a11, a22), np.multiply(a12, a12))
        Xn, Yn = Xp + Dx, Yp + Dy
        if not _inside(Xn, Yn, W, H):
            return lost(LOST_FRAME, iters)
        for _ in range(max_iters):
            E = window(nxt[l], Xn, Yn, r) - P
            B1, B2 = int((E * gx).sum()), int((E * gy).sum())
            iters += 1
            b1, b2 = np.float64(B1), np.float64(B2)
            with np.errstate(all="ignore"):
                dx = np.divide(np.subtract(np.multiply(a12, b2), np.multiply(a22, b1)), det)
                dy = np.divide(np.subtract(np.multiply(a12, b1), np.multiply(a11, b2)), det)
            fdx, fdy = _round_step(dx), _round_step(dy)
            if trace is not None:
                trace[-1]["b"].append((B1, B2))
            if fdx is None or fdy is None:
                return lost(LOST_STEP, iters)
            Xn, Yn = Xn + fdx, Yn + fdy
            if trace is not None:
                trace[-1]["pos"].append((Xn, Yn))
            if not _inside(Xn, Yn, W, H):
                return lost(LOST_FRAME, iters)
            if abs(fdx) + abs(fdy) <= eps:
                break
        Dx, Dy = Xn - Xp, Yn - Yp
    err = int(np.abs(window(nxt[0], Xn, Yn, r) - P).sum())
    return TRACKED, Xn, Yn, err, iters


def frame_range(offs, cap, f):
    b = min(int(offs[f]), cap)
    return b, max(min(int(offs[f + 1]), cap), b)


def track(prev_frames, next_frames, points, offs, cap, coords=COORDS_U32, keep=None, guess=None,
          radius=10, max_iters=30, eps=20, min_eig=1e-3):
    """The whole call.  ``prev_frames[f]`` / ``next_frames[f]`` are the level lists of frame f of
    the call; ``points`` is (cap, 2) (pixels for COORDS_U32, Q11 for COORDS_Q11).  Returns a dict of
    arrays of ``cap`` entries and the boolean mask ``written`` of the entries the call writes."""
    n = (2 * radius + 1) ** 2
    out = {
        "q11": np.zeros((cap, 2), np.int32), "f32": np.zeros((cap, 2), np.float32),
        "status": np.zeros(cap, np.uint8), "err": np.zeros(cap, np.uint32),
        "info": np.zeros(cap, np.uint32), "matches": np.zeros((cap, 2), np.uint32),
        "written": np.zeros(cap, bool),
    }
    pts = np.asarray(points).reshape(-1, 2)
    for f in range(len(prev_frames)):
        lo, hi = frame_range(offs, cap, f)
        for i in range(lo, hi):
            if coords == COORDS_U32:
                x, y = int(pts[i, 0]), int(pts[i, 1])
                # x * 2048 of a u32 that would leave int32 is outside every frame
                X, Y = (x * ONE if x < (1 << 20) else -1), (y * ONE if y < (1 << 20) else -1)
            else:
                X, Y = int(np.int32(pts[i, 0])), int(np.int32(pts[i, 1]))
            if keep is not None and keep[i] == 0:
                res = (SKIPPED, -1, -1, NO_ERR, 0)
            else:
                g = None if guess is None else (int(guess[i][0]), int(guess[i][1]))
                res = track_point(prev_frames[f], next_frames[f], X, Y, g, radius, max_iters, eps,
                                  min_eig)
            reason, Xn, Yn, err, iters = res
            out["written"][i] = True
            out["q11"][i] = (Xn, Yn)
            out["info"][i] = reason | iters << 8
            out["err"][i] = err
            if reason == TRACKED:
                out["f32"][i] = (np.float32(np.float64(Xn) / 2048.0), np.float32(np.float64(Yn) / 2048.0))
                out["status"][i] = 1
                out["matches"][i] = (i, min(err // n, 0xFFFE) | 0xFFFF << 16)
            else:
                out["f32"][i] = (-1.0, -1.0)
                out["matches"][i] = (MATCH_NONE, 0xFFFF | 0xFFFF << 16)
    return out


def worked_frames():
    """The 32 x 24 frames A and B of the header's worked example."""
    x = np.arange(32, dtype=np.int64)[None, :]
    y = np.arange(24, dtype=np.int64)[:, None]
    a = np.minimum(255, ((x - 16) ** 2 + 2 * (y - 12) ** 2 + (x - 16) * (y - 12)) >> 2).astype(np.uint8)
    b = a[np.clip(y - 1, 0, 23), np.clip(x - 2, 0, 31)]
    return a, b
