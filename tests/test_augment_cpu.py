"""CPU: the augmentation's host side (vistaocr_amd/augment.py: the draw, the tables, the hook in fit()), the numpy restatement
(tests/augment_ref.py) against scipy, and the argument validation of the two entry points, which needs no device."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import augment_ref as ar

ALL_ON = dict(p_rotate=1.0, p_crop_x=1.0, p_crop_y=1.0, p_pad=1.0, p_shift=1.0, p_filter_ones=0.5, p_filter_rand=0.5, p_contrast=1.0,
              p_invert=1.0, p_mesh=1.0, p_noise=1.0, p_delete=1.0, p_stripe=1.0)


def test_restated_geometry_equals_scipy_map_coordinates():
    """Stage 1 of the restatement in fp64 against scipy.ndimage.map_coordinates(order=1, mode="nearest") at the same coordinates:
    rotation, zoom and shift on a 7 x 33 image, the map leaving the image on every side."""
    from scipy.ndimage import map_coordinates
    from vistaocr_amd.augment import compose_affine
    rng = np.random.default_rng(3)
    h, w = 7, 33
    img = rng.random((h, w))
    a = compose_affine(w, h, angle_deg=7.0, zoom_x=1.3, zoom_y=0.8, shift_x=-1.1, shift_y=1.3)
    rec = ar.make_params(1, A=a.reshape(-1))[0]
    mine = ar.geometry(img[None], rec, w, None, 0, np.float64)[0]
    oy, ox = np.mgrid[0:h, 0:w].astype(np.float64)
    a64 = a.astype(np.float64)
    xs = a64[0, 0] * ox + (a64[0, 1] * oy + a64[0, 2])
    ys = a64[1, 0] * ox + (a64[1, 1] * oy + a64[1, 2])
    assert xs.min() < -1 and xs.max() > w and ys.min() < -0.5 and ys.max() > h - 0.5      # the border rule is exercised
    ref = map_coordinates(img, [ys, xs], order=1, mode="nearest")
    assert np.abs(mine - ref).max() <= 1e-12


def test_draw_is_a_function_of_seed_step_and_line_only():
    from vistaocr_amd.augment import DeviceAugmenter
    aug = DeviceAugmenter(seed=5, **ALL_ON)
    widths = [200, 150, 90, 60, 31]
    full = aug.draw(widths, 30, step=3)
    again = aug.draw(widths, 30, step=3)
    assert np.array_equal(full.records, again.records) and np.array_equal(full.mesh, again.mesh)
    for i, w in enumerate(widths):                      # line i alone, at position i of a batch of i + 1 lines: the same draw
        part = aug.draw(widths[:i + 1], 30, step=3)
        assert np.array_equal(part.records[i], full.records[i])
        gw = int(part.records[i, 18])
        assert np.array_equal(part.mesh[i, :, :, :gw + 1], full.mesh[i, :, :, :gw + 1])
        assert not part.mesh[i, :, :, gw + 1:].any()
    other = aug.draw(widths, 30, step=4)
    assert not np.array_equal(other.records[:, :6], full.records[:, :6])
    assert not np.array_equal(DeviceAugmenter(seed=6, **ALL_ON).draw(widths, 30, 3).records[:, 21:23], full.records[:, 21:23])
    assert len({tuple(r) for r in full.records[:, 21:23]}) == len(widths)                # every line its own noise key
    # ranks of a data-parallel job draw different streams
    a0, a1 = DeviceAugmenter(seed=5, **ALL_ON).seed_rank(0), DeviceAugmenter(seed=5, **ALL_ON).seed_rank(1)
    assert np.array_equal(a0.draw(widths, 30, 3).records, full.records)
    assert not np.array_equal(a1.draw(widths, 30, 3).records, full.records)


def test_every_drawn_parameter_lies_in_its_range():
    from vistaocr_amd.augment import DeviceAugmenter, FLAG_FILTER, FLAG_INVERT, FLAG_MESH
    opts = dict(ALL_ON, rotate_deg=(-3.0, 1.0), crop_x=0.04, crop_y=0.2, pad_x=0.0, pad_y=0.0, p_pad=0.0, shift_x=(-5.0, -1.0),
                shift_y=(0.5, 2.0), contrast=(0.7, 1.5), mesh_interval=(40.0, 12.0), mesh_std=(2.0, 0.5), noise_p=0.25,
                noise_sigma=0.1, delete_p=0.125, delete_value=0.75, stripe_rows=(2, 5), stripe_value=0.25)
    aug = DeviceAugmenter(seed=11, **opts)
    h = 30
    widths = np.arange(400, 0, -1)
    p = aug.draw(widths, h, step=0)
    d, f = p.drawn, p.records.view(np.float32)
    assert ((d["angle_deg"] >= -3.0) & (d["angle_deg"] <= 1.0)).all()
    assert ((d["crop_x"] >= 0) & (d["crop_x"] <= 0.04) & (d["crop_y"] >= 0) & (d["crop_y"] <= 0.2)).all()
    assert ((d["shift_x"] >= -5.0) & (d["shift_x"] <= -1.0) & (d["shift_y"] >= 0.5) & (d["shift_y"] <= 2.0)).all()
    assert ((f[:, 11] >= np.float32(0.7)) & (f[:, 11] <= np.float32(1.5))).all()
    assert (p.records[:, 17] & (FLAG_MESH | FLAG_FILTER | FLAG_INVERT) == 7).all()
    assert p.gh == 2 and (p.records[:, 18].astype(np.int64) == np.maximum(1, np.rint(widths / 40.0))).all()     # round(30 / 12) = 2
    assert p.mesh.shape == (400, 2, 3, 11) and np.abs(p.mesh[:, 0]).max() < 6 * 2.0 and np.abs(p.mesh[:, 1]).max() < 6 * 0.5
    assert abs(p.mesh[:40, 0].std() / 2.0 - 1) < 0.1 and abs(p.mesh[:40, 1].std() / 0.5 - 1) < 0.1     # (the widest lines use every node)
    assert (f[:, 12] == np.float32(0.25)).all() and (f[:, 13] == np.float32(0.1)).all()
    assert (f[:, 14] == np.float32(0.125)).all() and (f[:, 15] == np.float32(0.75)).all() and (f[:, 16] == np.float32(0.25)).all()
    r0, r1 = p.records[:, 19].astype(np.int64), p.records[:, 20].astype(np.int64)
    assert ((r0 >= 0) & (r0 < h) & (r1 > r0) & (r1 <= h) & (r1 - r0 <= 5)).all()
    assert ((d["stripe_rows"] >= 2) & (d["stripe_rows"] <= 5)).all() and set(d["stripe_rows"]) == {2.0, 3.0, 4.0, 5.0}
    taps = f[:, 6:11]
    ones = d["filter"] == 1
    assert (taps[ones] == 1.0).all() and np.abs(taps[~ones]).max() < 6.0 and 0.8 < taps[~ones].std() < 1.2
    # the affine map is the fp32 rounding of the fp64 composition of what was drawn
    from vistaocr_amd.augment import compose_affine
    for i in (0, 17, 399):
        want = compose_affine(int(widths[i]), h, d["angle_deg"][i], d["zoom_x"][i], d["zoom_y"][i], d["shift_x"][i], d["shift_y"][i])
        assert np.array_equal(f[i, 0:6], want.reshape(-1))
    # the composition itself: the centre is a fixed point of a pure rotation / zoom, a shift moves it
    a = compose_affine(100, 30, angle_deg=2.0, zoom_x=0.9, zoom_y=1.1).astype(np.float64)
    assert np.allclose(a @ np.array([50.0, 15.0, 1.0]), [50.0, 15.0], atol=1e-5)
    a = compose_affine(100, 30, angle_deg=90.0).astype(np.float64)
    assert np.allclose(a[:, :2], [[0, -1], [1, 0]], atol=1e-7)
    assert np.allclose(compose_affine(100, 30, shift_x=3, shift_y=-1), [[1, 0, 3], [0, 1, -1]])


def test_all_probabilities_zero_encode_the_identity():
    from vistaocr_amd.augment import DeviceAugmenter, make_records
    p = DeviceAugmenter(seed=9).draw([300, 20, 1], 30, step=7)
    want = make_records(3)
    assert np.array_equal(p.records[:, :21], want[:, :21]) and p.mesh is None and not p.with_filter and (p.gh, p.gw_max) == (0, 0)
    f = p.records.view(np.float32)
    assert np.array_equal(f[0, 0:6], np.float32([1, 0, 0, 0, 1, 0])) and f[0, 11] == 1.0
    assert not f[:, 12].any() and not f[:, 14].any() and not p.records[:, 17].any() and not p.records[:, 19:21].any()
    # and the restatement maps such tables to the identity, pad columns zeroed
    x = np.random.default_rng(0).random((3, 1, 30, 300)).astype(np.float32)
    y = ar.augment(x, p.widths, p.records)
    for i, w in enumerate((300, 20, 1)):
        assert np.array_equal(y[i, :, :, :w], x[i, :, :, :w].astype(np.float64)) and not y[i, :, :, w:].any()
    buf, (o_rec, o_mesh) = p.packed()
    assert buf.dtype == np.int32 and o_rec % 4 == 0 and buf.size == o_mesh and np.array_equal(buf[:3], [300, 20, 1])
    assert np.array_equal(buf[o_rec:o_mesh].view(np.uint32).reshape(3, 24), p.records)


def test_preset_frequencies_match_the_reference_probabilities():
    """--synth_input / --stripe (src/train_cnn_lstm.py:207-274): on / off frequencies over 4000 draws within 4 binomial standard
    deviations of the reference's probabilities."""
    from vistaocr_amd.augment import DeviceAugmenter
    n = 4000
    aug = DeviceAugmenter.synth_input(stripe=True, seed=1)
    d = aug.draw(np.full(n, 200), 30, step=0).drawn
    got = dict(rotate=np.isfinite(d["angle_deg"]).mean(), ones=(d["filter"] == 1).mean(), rand=(d["filter"] == 2).mean(),
               identity=(d["filter"] == 0).mean(), contrast=np.isfinite(d["alpha"]).mean(), crop_x=np.isfinite(d["crop_x"]).mean(),
               crop_y=np.isfinite(d["crop_y"]).mean(), stripe=np.isfinite(d["stripe_r0"]).mean(), mesh=d["mesh"].mean(),
               noise=d["noise"].mean(), delete=d["delete"].mean(), invert=d["invert"].mean())
    want = dict(rotate=0.3, ones=1 / 3, rand=1 / 3, identity=1 / 3, contrast=0.5, crop_x=0.2, crop_y=0.2, stripe=0.3, mesh=0.0,
                noise=0.0, delete=0.0, invert=0.0)
    for k, p in want.items():
        assert abs(got[k] - p) <= 4 * math.sqrt(p * (1 - p) / n), (k, got[k], p)
    ang, al = d["angle_deg"][np.isfinite(d["angle_deg"])], d["alpha"][np.isfinite(d["alpha"])]
    assert -2 <= ang.min() < -1.9 and 1.9 < ang.max() <= 2 and 0.5 <= al.min() < 0.52 and 1.97 < al.max() <= 2.0
    cx, cy = d["crop_x"][np.isfinite(d["crop_x"])], d["crop_y"][np.isfinite(d["crop_y"])]
    assert 0 <= cx.min() and 0.049 < cx.max() <= 0.05 and 0 <= cy.min() and 0.098 < cy.max() <= 0.1
    assert set(d["stripe_rows"][np.isfinite(d["stripe_rows"])]) == {1.0, 2.0, 3.0, 4.0}
    assert np.isfinite(DeviceAugmenter.synth_input(seed=1).draw(np.full(n, 200), 30, 0).drawn["stripe_r0"]).sum() == 0   # --stripe off


def test_non_finite_and_degenerate_parameters_raise():
    from vistaocr_amd.augment import AugmentParams, DeviceAugmenter, compose_affine, make_records
    for bad in (dict(rotate_deg=(float("nan"), 2.0)), dict(contrast=(0.5, float("inf"))), dict(noise_sigma=float("nan")),
                dict(p_rotate=1.5), dict(crop_x=0.5), dict(mesh_interval=(0.0, 25.0)), dict(p_filter_ones=0.7, p_filter_rand=0.7)):
        with pytest.raises(ValueError):
            DeviceAugmenter(seed=0, **bad)
    with pytest.raises(TypeError):
        DeviceAugmenter(seed=0, p_emboss=0.3)
    for bad in (dict(angle_deg=float("nan")), dict(zoom_x=0.0), dict(zoom_y=-1.0), dict(shift_x=float("inf")), dict(zoom_x=1e39)):
        with pytest.raises(ValueError):
            compose_affine(100, 30, **bad)
    rec = make_records(2)
    rec.view(np.float32)[1, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        AugmentParams([5, 4], 30, rec, None, 0, 0)
    with pytest.raises(ValueError):
        DeviceAugmenter(seed=0).draw([10, 0], 30, 0)


def test_fit_hands_train_fn_the_augmented_batch_and_leaves_validation_alone(tmp_path):
    import torch
    import vistaocr_amd as va
    from vistaocr_amd.loop import fit
    m = va.CnnOcrModel(alphabet=va.english_alphabet(), gpu=False, verbose=False, input_line_height=30, rds_line_height=30,
                       lstm_input_dim=16, num_lstm_layers=1, num_lstm_hidden_units=16, p_lstm_dropout=0.0)
    opt = va.FlatClampAdam(m.parameters(), lr=1e-3)
    seen_train, seen_val, calls = [], [], []

    def stub_augmenter(batch):
        calls.append(batch)
        return ("augmented", batch)

    def fake_train(batch, model, crit, optimizer):
        seen_train.append(batch)
        return 32.0

    def fake_val(loader, model, crit):
        seen_val.extend(loader)
        return 1.0, 0.5, 0.5
    train_batches, val_batches = ["t%d" % i for i in range(6)], ["v0", "v1"]
    prefix = os.path.join(tmp_path, "run")
    fit(m, None, opt, train_batches, val_batches, fake_train, prefix, batch_size=32, snapshot_every_n_iterations=3, validate_fn=fake_val,
        augmenter=stub_augmenter)
    assert calls == train_batches and seen_train == [("augmented", b) for b in train_batches]
    assert seen_val == val_batches * 2
    seen_train.clear()
    fit(m, None, opt, train_batches, val_batches, fake_train, prefix, batch_size=32, snapshot_every_n_iterations=3, validate_fn=fake_val)
    assert seen_train == train_batches                                                  # augmenter=None: today's behaviour
    assert torch.is_tensor(next(m.parameters()))


def test_entry_points_validate_their_arguments_without_a_device():
    from vistaocr_amd import _lib
    lib = _lib.load()
    one, two = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)

    def call(x=one, widths=one, b=2, c=1, h=30, wmax=64, params=one, mesh=None, gh=0, gw_max=0, with_filter=1, y=two, ws=one, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = lib.vocr_augment_workspace_bytes(b, c, h, wmax)
        return lib.vocr_augment_lines(x, widths, b, c, h, wmax, params, mesh, gh, gw_max, with_filter, y, ws, ws_bytes, None)

    def refused(needle=b"", **kw):
        rc, msg = call(**kw), lib.vocr_last_error()
        return rc == -1 and b"vocr_augment_lines" in msg and needle in msg

    assert lib.vocr_augment_workspace_bytes(32, 1, 30, 600) == 32 * 4 * 3 * 8 and lib.vocr_augment_workspace_bytes(1, 3, 60, 1200) == 3 * 8 * 5 * 8
    for bad in ((0, 1, 30, 64), (2, 0, 30, 64), (2, 1, 0, 64), (2, 1, 30, 0), (2, 2, 30, 64), (2, 4, 30, 64), (-1, 1, 30, 64)):
        assert lib.vocr_augment_workspace_bytes(*bad) == 0
    for name in ("x", "widths", "params", "y"):
        assert refused(b"null pointer", **{name: None})
    assert refused(b"null pointer", ws=None)
    assert refused(b"8-byte aligned", ws=ctypes.c_void_p((1 << 20) + 4))
    for name in ("b", "h", "wmax"):
        assert refused(b">= 1", ws_bytes=1 << 20, **{name: 0}) and refused(b">= 1", ws_bytes=1 << 20, **{name: -3})
    assert refused(b">= 1", c=0, ws_bytes=1 << 20)
    assert refused(b"1 or 3", c=2, ws_bytes=1 << 20) and refused(b"1 or 3", c=4, ws_bytes=1 << 20)
    assert refused(b"in place", y=one)
    assert refused(b"in place", y=ctypes.c_void_p((1 << 20) + 4 * 2 * 30 * 64 - 4))       # y begins inside x
    assert refused(b"workspace too small", ws_bytes=lib.vocr_augment_workspace_bytes(2, 1, 30, 64) - 1)
    assert refused(b"mesh", mesh=one, gh=0, gw_max=3) and refused(b"mesh", mesh=one, gh=1, gw_max=0)
