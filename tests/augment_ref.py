"""numpy restatement of vocr_augment_lines (include/vocr.h), stage by stage, in a float type of the caller's choice: float64 is the
reference, float32 - the same operations in the same order, every multiply-add rounded twice - measures what fp32 costs on a test's
own inputs (the kernel's bar is a multiple of that).  The integer hash runs in uint64 arithmetic.  Tables in the header's layout."""
import numpy as np

REC = 24
FLAG_MESH, FLAG_FILTER, FLAG_INVERT = 1, 2, 4
_G = np.uint64(0x9e3779b97f4a7c15)


def make_params(b, **fields):
    """uint32 [b, 24] identity records with `fields` set for every line (scalars or [b] arrays): A (six floats, [6] or [b, 6]), taps
    ([5]: k00 k01 k10 k11 bias), alpha, p_noise, sigma, p_del, del_value, stripe_value, flags, gw, r0, r1, key."""
    r = np.zeros((b, REC), dtype=np.uint32)
    f = r.view(np.float32)
    f[:, 0] = f[:, 4] = f[:, 9] = f[:, 11] = 1.0
    r[:, 18] = 1
    where = dict(alpha=11, p_noise=12, sigma=13, p_del=14, del_value=15, stripe_value=16)
    for k, v in fields.items():
        if k == "A":
            f[:, 0:6] = np.asarray(v, dtype=np.float32).reshape(-1, 6)
        elif k == "taps":
            f[:, 6:11] = np.asarray(v, dtype=np.float32).reshape(-1, 5)
        elif k in where:
            f[:, where[k]] = np.asarray(v, dtype=np.float32)
        elif k in ("flags", "gw", "r0", "r1"):
            r[:, dict(flags=17, gw=18, r0=19, r1=20)[k]] = np.asarray(v, dtype=np.int64).astype(np.uint32)
        elif k == "key":
            key = np.asarray(v, dtype=np.uint64) * np.ones(b, dtype=np.uint64)
            r[:, 21] = (key & np.uint64(0xffffffff)).astype(np.uint32)
            r[:, 22] = (key >> np.uint64(32)).astype(np.uint32)
        else:
            raise KeyError(k)
    return r


def aug_bits(key, ch, oy, ox, draw):
    """uint32 array: the upper half of the splitmix64 finaliser of key * G + (ox | oy << 24 | ch << 48 | draw << 56), as the header says."""
    u = lambda v: np.asarray(v, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = u(key) * _G + (u(ox) | (u(oy) << u(24)) | (u(ch) << u(48)) | (u(draw) << u(56)))
        z = (z ^ (z >> u(30))) * u(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> u(27))) * u(0x94d049bb133111eb)
        z = z ^ (z >> u(31))
    return (z >> u(32)).astype(np.uint32)


def uniform24(bits, plus_one=False):
    """float64 (exact): (bits >> 8) * 2^-24, or ((bits >> 8) + 1) * 2^-24"""
    return ((bits >> np.uint32(8)).astype(np.float64) + (1.0 if plus_one else 0.0)) * 2.0 ** -24


def _lerp(a, b, t):
    return t * (b - a) + a


def source_coords(rec, w, h, mesh_b, gh, dt):
    """(xs, ys) [h, w] in dt: stage 1's clamped source coordinates of one line (record `rec`, uint32 [24])."""
    f = rec[:17].view(np.float32).astype(dt)
    oy, ox = np.mgrid[0:h, 0:w]
    px, py = ox.astype(dt), oy.astype(dt)
    if (int(rec[17]) & FLAG_MESH) and mesh_b is not None:
        gw = min(max(int(np.int32(rec[18])), 1), mesh_b.shape[2] - 1)
        sx, sy = dt(gw) / dt(w), dt(gh) / dt(h)
        u, v = px * sx, py * sy
        j, i = np.minimum(np.floor(u).astype(np.int64), gw - 1), np.minimum(np.floor(v).astype(np.int64), gh - 1)
        fu, fv = u - j.astype(dt), v - i.astype(dt)
        d = []
        for plane in range(2):
            m = mesh_b[plane].astype(dt)
            d.append(_lerp(_lerp(m[i, j], m[i, j + 1], fu), _lerp(m[i + 1, j], m[i + 1, j + 1], fu), fv))
        px, py = px + d[0], py + d[1]
    xs = f[0] * px + (f[1] * py + f[2])
    ys = f[3] * px + (f[4] * py + f[5])
    return np.minimum(np.maximum(xs, dt(0)), dt(w - 1)), np.minimum(np.maximum(ys, dt(0)), dt(h - 1))


def bilinear(img, xs, ys, dt):
    """img [h, w] sampled at (xs, ys) (already clamped): taps floor and min(floor + 1, limit)."""
    h, w = img.shape
    img = img.astype(dt)
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = xs - x0.astype(dt), ys - y0.astype(dt)
    return _lerp(_lerp(img[y0, x0], img[y0, x1], fx), _lerp(img[y1, x0], img[y1, x1], fx), fy)


def geometry(xl, rec, w, mesh_b, gh, dt):
    """R [c, h, w]: stage 1 of one line; xl [c, h, >= w] (only [:w] is read)."""
    xs, ys = source_coords(rec, w, xl.shape[1], mesh_b, gh, dt)
    return np.stack([bilinear(xl[ch, :, :w], xs, ys, dt) for ch in range(xl.shape[0])])


def block_filter(r, rec, dt):
    """stage 2 on R [c, h, w]: the 2x2 filter with zero padding and the renormalisation over the whole line."""
    f = rec[:17].view(np.float32).astype(dt)
    p = np.zeros((r.shape[0], r.shape[1] + 1, r.shape[2] + 1), dtype=dt)
    p[:, 1:, 1:] = r
    ul, uc, rl, rc = p[:, :-1, :-1], p[:, :-1, 1:], p[:, 1:, :-1], p[:, 1:, 1:]
    F = (((f[10] + f[6] * ul) + f[7] * uc) + f[8] * rl) + f[9] * rc
    mn, mx = F.min(), F.max()
    den = mx - mn
    return (F - mn) / den if den > 0 else np.zeros_like(F)


def decisions(rec, c, h, w):
    """(noised, deleted) bool [c, h, w] of one line: exact, whatever the float type."""
    f = rec.view(np.float32)
    key = np.uint64(rec[21]) | (np.uint64(rec[22]) << np.uint64(32))
    ch, oy, ox = np.mgrid[0:c, 0:h, 0:w]
    noised = uniform24(aug_bits(key, ch, oy, ox, 0)) < np.float64(f[12])
    deleted = uniform24(aug_bits(key, ch, oy, ox, 3)) < np.float64(f[14])
    return noised, deleted


def photometric(v, rec, dt):
    """stage 3 on v [c, h, w]"""
    f = rec[:17].view(np.float32).astype(dt)
    c, h, w = v.shape
    key = np.uint64(rec[21]) | (np.uint64(rec[22]) << np.uint64(32))
    ch, oy, ox = np.mgrid[0:c, 0:h, 0:w]
    if rec.view(np.float32)[11] != 1.0:
        v = (v - dt(0.5)) * f[11] + dt(0.5)
    if int(rec[17]) & FLAG_INVERT:
        v = dt(1) - v
    noised, deleted = decisions(rec, c, h, w)
    u1 = uniform24(aug_bits(key, ch, oy, ox, 1), plus_one=True).astype(dt)
    u2 = uniform24(aug_bits(key, ch, oy, ox, 2)).astype(dt)
    n = np.sqrt(dt(-2) * np.log(u1)) * np.cos(dt(2 * np.pi) * u2)
    v = np.where(noised, f[13] * n + v, v)
    v = np.where(deleted, f[15], v)
    r0, r1 = int(np.int32(rec[19])), int(np.int32(rec[20]))
    rows = (oy >= r0) & (oy < r1)
    v = np.where(rows, f[16], v)
    return np.minimum(np.maximum(v, dt(0)), dt(1)).astype(dt)


def augment(x, widths, params, mesh=None, gh=0, dt=np.float64):
    """y [b, c, h, wmax] in dt: all four stages.  x [b, c, h, wmax] (the pad columns are never read), params uint32 [b, 24], mesh
    fp32 [b, 2, gh + 1, gw_max + 1] or None."""
    b, c, h, wmax = x.shape
    y = np.zeros(x.shape, dtype=dt)
    for i in range(b):
        w = int(min(max(int(widths[i]), 0), wmax))
        if w == 0:
            continue
        rec = np.ascontiguousarray(params[i])
        v = geometry(x[i], rec, w, None if mesh is None else mesh[i], gh, dt)
        if int(rec[17]) & FLAG_FILTER:
            v = block_filter(v, rec, dt)
        y[i, :, :, :w] = photometric(v, rec, dt)
    return y
