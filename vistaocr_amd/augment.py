"""Training augmentation on the device (include/vocr.h: vocr_augment_lines): the chain the reference applies per image in its
DataLoader workers with OpenCV, imgaug and scipy (src/train_cnn_lstm.py:203-274, src/imagetransforms.py:71-406), applied to the
collated batch in one gather.

    aug = DeviceAugmenter.synth_input(stripe=True, seed=7)
    fit(model, criterion, optimizer, train_loader, val_loader, train, prefix, batch_size, augmenter=aug)

All randomness is drawn HERE, on the host, in pure numpy (`draw`): line i of step s gets a deterministic function of (seed, s, i),
whatever the batch size.  The kernel is a pure function of the tables `draw` returns.

What differs from the reference, on purpose:
  * WIDTHS DO NOT CHANGE.  The model needs its widths sorted descending and derives the LSTM's lengths from them, so every line keeps
    its own box.  CropHorizontal / CropVertical (a symmetric chop of up to 5 % / 10 %) become a zoom INTO the box about its centre
    (zoom factor 1 - 2 pct), PadRandom a zoom out with border replicate and a shift; neither becomes a new width.
  * The mesh warp interpolates its control grid bilinearly (the reference: scipy's Delaunay griddata over the scattered nodes).
  * No quantisation to uint8 anywhere; the block filter's renormalisation gives 0 for a constant line (the reference divides by zero).
  * One contrast factor per line (imgaug's per_channel=0.5 is not built); imgaug's Grayscale and Emboss are not built.
  * No parity claim against OpenCV or imgaug: neither is a dependency."""
import math

import numpy as np
import torch

REC_WORDS = 24                      # include/vocr.h: words of a line's record
FLAG_MESH, FLAG_FILTER, FLAG_INVERT = 1, 2, 4
_G = np.uint64(0x9e3779b97f4a7c15)
_M64 = (1 << 64) - 1

# slots of a line's uniform stream (slot 0 is the kernel's noise key); mesh node n uses _S_MESH + 2 n, + 1
(_S_KEY, _S_ROT, _S_ANGLE, _S_CROPX, _S_CROPX_V, _S_CROPY, _S_CROPY_V, _S_PAD, _S_PAD_L, _S_PAD_R, _S_PAD_T, _S_PAD_B, _S_SHIFT,
 _S_SHIFT_X, _S_SHIFT_Y, _S_FILTER, _S_CONTRAST, _S_ALPHA, _S_INVERT, _S_MESH_ON, _S_NOISE, _S_DELETE, _S_STRIPE, _S_STRIPE_AT,
 _S_STRIPE_ROWS) = range(25)
_S_TAPS = 32                        # 10 slots: five normals
_S_MESH = 64


def _mix64(z):
    """splitmix64's finaliser on a uint64 array (the hash of vocr_dropout_fwd, all 64 bits)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def _line_keys(seed, step, lines):
    """uint64 [len(lines)]: the stream key of line i at (seed, step) - nothing else enters a line's draw."""
    lines = np.asarray(lines, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = _mix64(np.full(lines.shape, int(seed) & _M64, dtype=np.uint64) * _G)
        k = _mix64(k ^ np.uint64(int(step) & _M64))
        return _mix64((k + _G) ^ lines)


def _bits(keys, slots):
    """uint64 draws of stream `keys` [n] at `slots` (broadcast against keys)."""
    with np.errstate(over="ignore"):
        return _mix64(keys + (np.asarray(slots, dtype=np.uint64) + np.uint64(1)) * _G)


def _uniform(keys, slots):
    """fp64 uniforms in [0, 1) with 53 bits."""
    return (_bits(keys, slots) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _normal(keys, slots):
    """fp64 standard normals (Box-Muller); each uses slots s and s + 1."""
    s = np.asarray(slots, dtype=np.uint64)
    return np.sqrt(-2.0 * np.log(1.0 - _uniform(keys, s))) * np.cos(2.0 * math.pi * _uniform(keys, s + np.uint64(1)))


def compose_affine(w, h, angle_deg=0.0, zoom_x=1.0, zoom_y=1.0, shift_x=0.0, shift_y=0.0):
    """The inverse map (output pixel indices -> source pixel indices) of one line as fp32 [2, 3], composed in fp64:
    p_src = c + shift + Rot(angle) diag(zoom) (p_out - c), c = (w / 2, h / 2) - the centre cv2.getRotationMatrix2D is given by the
    reference.  zoom < 1 looks INTO the line (a crop), zoom > 1 shows its replicated border (a pad).  Raises ValueError for a
    non-finite parameter or a zoom that is not positive."""
    vals = (float(angle_deg), float(zoom_x), float(zoom_y), float(shift_x), float(shift_y))
    if not all(math.isfinite(v) for v in vals) or w < 1 or h < 1:
        raise ValueError("compose_affine: non-finite parameter or empty box: w=%r h=%r %r" % (w, h, vals))
    if vals[1] <= 0.0 or vals[2] <= 0.0:
        raise ValueError("compose_affine: degenerate zoom (%r, %r)" % (vals[1], vals[2]))
    th = math.radians(vals[0])
    cs, sn = math.cos(th), math.sin(th)
    cx, cy = w / 2.0, h / 2.0
    m = np.array([[cs * vals[1], -sn * vals[2]], [sn * vals[1], cs * vals[2]]], dtype=np.float64)
    t = np.array([cx + vals[3], cy + vals[4]]) - m @ np.array([cx, cy])
    with np.errstate(over="ignore"):
        a = np.concatenate([m, t[:, None]], axis=1).astype(np.float32)
    if not np.isfinite(a).all():
        raise ValueError("compose_affine: the map overflows fp32")
    return a


class AugmentParams(object):
    """The host tables of one batch (DeviceAugmenter.draw): `widths` int32 [B], `height`, `records` uint32 [B, 24] and `mesh` fp32
    [B, 2, gh + 1, gw_max + 1] or None in the layout of include/vocr.h, `gh`, `gw_max`, `with_filter`; `drawn`: what was drawn, by
    name, float64 [B] each (NaN where the step is off for the line)."""

    def __init__(self, widths, height, records, mesh, gh, gw_max, drawn=None):
        self.widths = np.ascontiguousarray(widths, dtype=np.int32)
        self.height = int(height)
        self.records = np.ascontiguousarray(records, dtype=np.uint32)
        self.mesh = None if mesh is None else np.ascontiguousarray(mesh, dtype=np.float32)
        self.gh, self.gw_max = (int(gh), int(gw_max)) if mesh is not None else (0, 0)
        self.drawn = drawn or {}
        b = self.widths.shape[0]
        if self.records.shape != (b, REC_WORDS):
            raise ValueError("AugmentParams: records must be [%d, %d], got %r" % (b, REC_WORDS, self.records.shape))
        if self.mesh is not None and self.mesh.shape != (b, 2, self.gh + 1, self.gw_max + 1):
            raise ValueError("AugmentParams: mesh must be [%d, 2, %d, %d], got %r" % (b, self.gh + 1, self.gw_max + 1, self.mesh.shape))
        floats = self.records[:, :17].view(np.float32)
        if not np.isfinite(floats).all() or (self.mesh is not None and not np.isfinite(self.mesh).all()):
            raise ValueError("AugmentParams: non-finite parameter")
        self.with_filter = bool((self.records[:, 17] & FLAG_FILTER).any())

    def packed(self):
        """(int32 1-d array, offsets): widths, records and mesh in one buffer for one upload; every part starts 16-byte aligned."""
        b = self.widths.shape[0]
        o_rec = (b + 3) // 4 * 4
        o_mesh = o_rec + b * REC_WORDS
        n = o_mesh + (self.mesh.size if self.mesh is not None else 0)
        buf = np.zeros(n, dtype=np.int32)
        buf[:b] = self.widths
        buf[o_rec:o_mesh] = self.records.reshape(-1).view(np.int32)
        if self.mesh is not None:
            buf[o_mesh:] = self.mesh.reshape(-1).view(np.int32)
        return buf, (o_rec, o_mesh)


def make_records(b):
    """uint32 [b, 24] identity records: A = identity, taps (0, 0, 0, 1), contrast 1, everything else off."""
    r = np.zeros((b, REC_WORDS), dtype=np.uint32)
    f = r.view(np.float32)
    f[:, 0] = f[:, 4] = f[:, 9] = f[:, 11] = 1.0
    r[:, 18] = 1
    return r


_DEFAULTS = dict(
    p_rotate=0.0, rotate_deg=(-2.0, 2.0),                 # RotateRandom
    p_crop_x=0.0, crop_x=0.05, p_crop_y=0.0, crop_y=0.1,  # CropHorizontal / CropVertical: U(0, crop) chopped off both ends -> zoom in
    p_pad=0.0, pad_x=0.05, pad_y=0.1,                     # PadRandom: U(0, pad) of the box added to each side on its own -> zoom out + shift
    p_shift=0.0, shift_x=(-2.0, 2.0), shift_y=(-1.0, 1.0),  # a shift in pixels
    p_filter_ones=0.0, p_filter_rand=0.0,                 # TessBlockConv(1, 1) / TessBlockConv(rand=True); the rest of the mass: identity
    p_contrast=0.0, contrast=(0.5, 2.0),                  # ContrastNormalization, one factor per line
    p_invert=0.0,                                         # Invert
    p_mesh=0.0, mesh_interval=(25.0, 25.0), mesh_std=(3.0, 3.0),   # WarpImage (w, h)
    p_noise=0.0, noise_p=0.7, noise_sigma=20.0 / 255.0,   # UniformNoise: a line with probability p_noise, then every pixel with noise_p
    p_delete=0.0, delete_p=0.7, delete_value=1.0,         # UniformDelete
    p_stripe=0.0, stripe_rows=(1, 4), stripe_value=0.0,   # AddRandomStripe
)


class DeviceAugmenter(object):
    """Augment collated training batches on the device.  Every step is off by default; an option p_<step> is the probability that a
    line gets the step, the others its range (see _DEFAULTS above for the reference transform each one restates).  `seed`: the stream;
    `step` counts the batches drawn through __call__."""

    def __init__(self, seed=0, **options):
        unknown = set(options) - set(_DEFAULTS)
        if unknown:
            raise TypeError("DeviceAugmenter: unknown option(s) %s" % sorted(unknown))
        self.opt = dict(_DEFAULTS, **options)
        self.seed, self.step = int(seed), 0
        o = self.opt
        flat = []
        for k, v in o.items():
            flat += [float(x) for x in (v if isinstance(v, (tuple, list)) else (v,))]
        if not all(math.isfinite(x) for x in flat):
            raise ValueError("DeviceAugmenter: non-finite option")
        for k in o:
            if k.startswith("p_") and not 0.0 <= o[k] <= 1.0:
                raise ValueError("DeviceAugmenter: %s must be a probability" % k)
        if o["p_filter_ones"] + o["p_filter_rand"] > 1.0 + 1e-12:
            raise ValueError("DeviceAugmenter: p_filter_ones + p_filter_rand > 1")
        for k in ("rotate_deg", "shift_x", "shift_y", "contrast", "stripe_rows"):
            if len(o[k]) != 2 or o[k][0] > o[k][1]:
                raise ValueError("DeviceAugmenter: %s must be (lo, hi) with lo <= hi" % k)
        if not (0.0 <= o["crop_x"] < 0.5 and 0.0 <= o["crop_y"] < 0.5 and o["pad_x"] >= 0.0 and o["pad_y"] >= 0.0):
            raise ValueError("DeviceAugmenter: degenerate zoom: crops must lie in [0, 0.5), pads be >= 0")
        if min(o["mesh_interval"]) <= 0.0 or min(o["mesh_std"]) < 0.0 or o["noise_sigma"] < 0.0 or int(o["stripe_rows"][0]) < 0:
            raise ValueError("DeviceAugmenter: mesh_interval must be > 0, mesh_std, noise_sigma and stripe_rows >= 0")
        if not (0.0 <= o["noise_p"] <= 1.0 and 0.0 <= o["delete_p"] <= 1.0):
            raise ValueError("DeviceAugmenter: noise_p and delete_p must be probabilities")

    @classmethod
    def synth_input(cls, stripe=False, seed=0, **overrides):
        """The reference's --synth_input chain (src/train_cnn_lstm.py:207-255) with its probabilities and ranges, and --stripe's
        (:273-274) on request: rotate p = 0.3 in U(-2, 2) degrees; block filter: ones + bias 1, N(0, 1) taps, identity, a third each;
        contrast p = 0.5, alpha in U(0.5, 2); horizontal / vertical crop p = 0.2 each, up to 5 % / 10 %, as zoom; stripe p = 0.3, 1-4
        rows of value 0.  Not in it: imgaug's Grayscale and Emboss (not built) and the Invert branch next to them (p_invert is the
        option; the reference's chain inverts a line with probability 0.3 * (1 + 0.1) / 4).  Mesh warp, noise and delete stay off: the
        reference's training script does not enable them."""
        o = dict(p_rotate=0.3, rotate_deg=(-2.0, 2.0), p_filter_ones=1.0 / 3.0, p_filter_rand=1.0 / 3.0, p_contrast=0.5, contrast=(0.5, 2.0),
                 p_crop_x=0.2, crop_x=0.05, p_crop_y=0.2, crop_y=0.1, p_stripe=0.3 if stripe else 0.0, stripe_rows=(1, 4), stripe_value=0.0)
        o.update(overrides)
        return cls(seed=seed, **o)

    def seed_rank(self, rank, base=None):
        """Per-rank stream of a data-parallel replica, offset as train.seed_rank offsets the model's dropout stream."""
        self.seed = (self.seed if base is None else int(base)) + 1000003 * int(rank)
        return self

    # ------------------------------------------------------------------------------------------------------------ the draw
    def draw(self, widths, height, step):
        """AugmentParams for a batch of lines with these widths: pure numpy, line i a function of (seed, step, i) only."""
        o = self.opt
        widths = np.asarray(widths, dtype=np.int64).reshape(-1)
        b, h = widths.shape[0], int(height)
        if b < 1 or h < 1 or (widths < 1).any():
            raise ValueError("DeviceAugmenter.draw: need at least one line, height >= 1 and widths >= 1")
        keys = _line_keys(self.seed, step, np.arange(b))
        u = lambda slot: _uniform(keys, slot)
        on = lambda slot, p: u(slot) < p
        between = lambda slot, lo_hi: lo_hi[0] + (lo_hi[1] - lo_hi[0]) * u(slot)
        nan = np.full(b, np.nan)
        drawn = {}
        rec = make_records(b)
        recf = rec.view(np.float32)
        key_bits = _bits(keys, _S_KEY)
        rec[:, 21] = (key_bits & np.uint64(0xffffffff)).astype(np.uint32)
        rec[:, 22] = (key_bits >> np.uint64(32)).astype(np.uint32)

        # geometry
        rot = on(_S_ROT, o["p_rotate"])
        angle = np.where(rot, between(_S_ANGLE, o["rotate_deg"]), 0.0)
        cx_on, cy_on = on(_S_CROPX, o["p_crop_x"]), on(_S_CROPY, o["p_crop_y"])
        crop_x = np.where(cx_on, o["crop_x"] * u(_S_CROPX_V), 0.0)
        crop_y = np.where(cy_on, o["crop_y"] * u(_S_CROPY_V), 0.0)
        pad = on(_S_PAD, o["p_pad"])
        pl, pr = np.where(pad, o["pad_x"] * u(_S_PAD_L), 0.0), np.where(pad, o["pad_x"] * u(_S_PAD_R), 0.0)
        pt, pb = np.where(pad, o["pad_y"] * u(_S_PAD_T), 0.0), np.where(pad, o["pad_y"] * u(_S_PAD_B), 0.0)
        sh = on(_S_SHIFT, o["p_shift"])
        shift_x = np.where(sh, between(_S_SHIFT_X, o["shift_x"]), 0.0) + (pr - pl) / 2.0 * widths
        shift_y = np.where(sh, between(_S_SHIFT_Y, o["shift_y"]), 0.0) + (pb - pt) / 2.0 * h
        zoom_x, zoom_y = (1.0 - 2.0 * crop_x) * (1.0 + pl + pr), (1.0 - 2.0 * crop_y) * (1.0 + pt + pb)
        for i in np.nonzero(rot | cx_on | cy_on | pad | sh)[0]:
            recf[i, 0:6] = compose_affine(int(widths[i]), h, angle[i], zoom_x[i], zoom_y[i], shift_x[i], shift_y[i]).reshape(-1)
        drawn.update(angle_deg=np.where(rot, angle, nan), crop_x=np.where(cx_on, crop_x, nan), crop_y=np.where(cy_on, crop_y, nan),
                     zoom_x=zoom_x, zoom_y=zoom_y, shift_x=shift_x, shift_y=shift_y)

        # mesh
        mesh, gh, gw_max = None, 0, 0
        m_on = on(_S_MESH_ON, o["p_mesh"])
        gw = np.maximum(1, np.rint(widths / o["mesh_interval"][0])).astype(np.int64)          # Python's round(), as WarpImage
        if m_on.any():
            gh = max(1, int(round(h / o["mesh_interval"][1])))
            gw_max = int(gw[m_on].max())
            plane, gi, gj = np.meshgrid(np.arange(2), np.arange(gh + 1), np.arange(gw_max + 1), indexing="ij")
            node = ((((plane << 12) | gi) << 20) | gj).astype(np.uint64)
            z = _normal(keys[:, None, None, None], np.uint64(_S_MESH) + np.uint64(2) * node[None])
            std = np.array([o["mesh_std"][0], o["mesh_std"][1]]).reshape(1, 2, 1, 1)
            used = m_on[:, None, None, None] & (gj[None] <= gw[:, None, None, None])
            mesh = np.where(used, z * std, 0.0).astype(np.float32)
            rec[m_on, 17] |= FLAG_MESH
            rec[:, 18] = np.minimum(gw, gw_max).astype(np.uint32)
        drawn.update(mesh=m_on.astype(np.float64))

        # block filter
        pick = u(_S_FILTER)
        ones = pick < o["p_filter_ones"]
        rnd = ~ones & (pick < o["p_filter_ones"] + o["p_filter_rand"])
        taps = _normal(keys[:, None], np.uint64(_S_TAPS) + np.uint64(2) * np.arange(5, dtype=np.uint64)[None])
        recf[ones, 6:11] = 1.0
        recf[rnd, 6:11] = taps[rnd].astype(np.float32)
        rec[ones | rnd, 17] |= FLAG_FILTER
        drawn.update(filter=np.where(ones, 1.0, np.where(rnd, 2.0, 0.0)))

        # photometric
        c_on = on(_S_CONTRAST, o["p_contrast"])
        alpha = np.where(c_on, between(_S_ALPHA, o["contrast"]), 1.0)
        recf[:, 11] = alpha.astype(np.float32)
        inv = on(_S_INVERT, o["p_invert"])
        rec[inv, 17] |= FLAG_INVERT
        n_on, d_on = on(_S_NOISE, o["p_noise"]), on(_S_DELETE, o["p_delete"])
        recf[:, 12] = np.where(n_on, o["noise_p"], 0.0).astype(np.float32)
        recf[:, 13] = np.where(n_on, o["noise_sigma"], 0.0).astype(np.float32)
        recf[:, 14] = np.where(d_on, o["delete_p"], 0.0).astype(np.float32)
        recf[:, 15] = np.where(d_on, o["delete_value"], 0.0).astype(np.float32)
        s_on = on(_S_STRIPE, o["p_stripe"])
        recf[:, 16] = np.where(s_on, o["stripe_value"], 0.0).astype(np.float32)
        lo, hi = int(o["stripe_rows"][0]), int(o["stripe_rows"][1])
        r0 = np.minimum((u(_S_STRIPE_AT) * h).astype(np.int64), h - 1)
        rows = lo + np.minimum((u(_S_STRIPE_ROWS) * (hi - lo + 1)).astype(np.int64), hi - lo)
        r1 = np.minimum(h, r0 + rows)
        rec[:, 19] = np.where(s_on, r0, 0).astype(np.uint32)
        rec[:, 20] = np.where(s_on, r1, 0).astype(np.uint32)
        drawn.update(alpha=np.where(c_on, alpha, nan), invert=inv.astype(np.float64), noise=n_on.astype(np.float64),
                     delete=d_on.astype(np.float64), stripe_r0=np.where(s_on, r0, nan), stripe_rows=np.where(s_on, rows, nan))
        return AugmentParams(widths, h, rec, mesh, gh, gw_max, drawn)

    # ------------------------------------------------------------------------------------------------------------ the device
    def apply(self, x_dev, widths, params):
        """y = the augmented batch, a new device tensor shaped like `x_dev` [B, C, H, Wmax] (fp32, on the device).  `params`: an
        AugmentParams of the same lines (`widths` is checked against it).  One packed upload of the tables, then the launches; nothing
        waits for the device."""
        from . import ops
        w = np.asarray(widths, dtype=np.int64).reshape(-1)
        if x_dev.dim() != 4 or w.shape[0] != x_dev.shape[0] or not np.array_equal(w, params.widths) or params.height != x_dev.shape[2]:
            raise ValueError("DeviceAugmenter.apply: params were drawn for other lines than this batch")
        if int(w.max()) > x_dev.shape[3]:
            raise ValueError("DeviceAugmenter.apply: a width exceeds the batch's padded width")
        buf, (o_rec, o_mesh) = params.packed()
        dev = torch.from_numpy(buf).to(x_dev.device, non_blocking=True)
        mesh = dev[o_mesh:].view(torch.float32) if params.mesh is not None else None
        return ops.augment_lines(x_dev, dev[:w.shape[0]], dev[o_rec:o_mesh], mesh, params.gh, params.gw_max, params.with_filter)

    def __call__(self, batch):
        """The collater's 5-tuple with the augmented DEVICE tensor in place of the image tensor; advances `step`."""
        x, targets, widths, target_lens, meta = batch
        params = self.draw(widths, x.shape[2], self.step)
        y = self.apply(x.cuda(non_blocking=True), widths, params)
        self.step += 1
        return y, targets, widths, target_lens, meta
