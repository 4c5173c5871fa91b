"""CPU: mmdx.clahe's numpy `reference` (the definition the kernels are held to), the descriptor
table of `plan`, the bundle config and every documented limit.  Exact equality throughout."""
import json
import types

import numpy as np
import pytest

import mmdx
from mmdx import clahe as K

from clahe_cases import (case, mixed_batch, random_image, serial_redistribute, smooth_image,
                         two_level_image)


def _tiles_of(img, tiles, tw, th):
    """The extended plane cut into tiles, written with slices (independent of reshape tricks)."""
    tx, ty = tiles
    ext = np.pad(img, ((0, th * ty - img.shape[0]), (0, tw * tx - img.shape[1])), mode="reflect")
    return [[ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw] for i in range(tx)] for j in range(ty)]


# ----------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("shape,tiles,clip_limit", [
    ((16, 16), (2, 2), 2.0), ((29, 37), (4, 3), 2.0), ((30, 32), (8, 8), 2.0),
    ((96, 80), (8, 8), 0.5), ((96, 80), (8, 8), 40), ((224, 224), (8, 8), 2.0)])
def test_histograms_keep_the_area_and_luts_are_monotone(shape, tiles, clip_limit):
    img = random_image(shape, 31)
    tw, th, clip, lut_scale = K.geometry(*shape, float(clip_limit), tiles)
    hist = K.tile_histograms(img, tiles, tw, th)
    parts = _tiles_of(img, tiles, tw, th)
    for j in range(tiles[1]):
        for i in range(tiles[0]):
            want = np.bincount(parts[j][i].ravel(), minlength=256)
            assert np.array_equal(hist[j, i], want)
            # the closed form is OpenCV's serial loop
            assert K.redistribute(hist[j, i], clip).tolist() == serial_redistribute(want, clip)
    red = K.redistribute(hist, clip)
    assert (red.sum(-1) == tw * th).all()
    assert clip == 0 or red.max() <= clip + (tw * th) // 256 + 1
    _, luts = K.reference(img, clip_limit, tiles, return_luts=True)
    assert luts.shape == (tiles[1], tiles[0], 256) and luts.dtype == np.uint8
    assert (np.diff(luts.astype(np.int64), axis=-1) >= 0).all()
    assert (luts[..., -1] == 255).all()


def test_one_tile_without_clipping_is_global_equalisation():
    for shape in [(40, 56), (33, 47)]:
        img = random_image(shape, 32) // 3 + 20
        got = K.reference(img, 0, (1, 1))
        cdf = np.cumsum(np.bincount(img.ravel(), minlength=256)).astype(np.float32)
        lut = np.rint(cdf * (np.float32(255) / np.float32(img.size)))
        assert np.array_equal(got, lut[img].astype(np.uint8))


def test_constant_tile_maps_to_one_value():
    img = np.full((32, 48), 90, np.uint8)
    out, luts = K.reference(img, 2.0, (4, 4), return_luts=True)
    assert len(np.unique(out)) == 1
    assert (luts == luts[0, 0]).all()
    # area 96, clip 1: 95 counts are handed out, batch 0, res 95, step 2, bins 0, 2, ..., 188
    tw, th, clip, scale = K.geometry(32, 48, 2.0, (4, 4))
    assert (tw, th, clip) == (12, 8, 1)
    h = np.zeros(256, np.int64)
    h[0:190:2] += 1
    h[90] += 1                   # its own count clipped to 1, on top of its share as an even bin
    assert h.sum() == 96
    assert np.array_equal(K.redistribute(np.bincount([90] * 96, minlength=256), 1), h)
    assert out[0, 0] == np.rint(np.float32(h[:91].sum()) * scale)


def test_equal_channels_stay_equal_and_match_the_grey_result():
    grey = random_image((45, 52), 33)
    rgb = np.repeat(grey[:, :, None], 3, axis=2)
    out, luts = K.reference(rgb, 2.0, (4, 4), return_luts=True)
    want, want_luts = K.reference(grey, 2.0, (4, 4), return_luts=True)
    assert out.shape == rgb.shape and luts.shape == (3, 4, 4, 256)
    for ch in range(3):
        assert np.array_equal(out[:, :, ch], want)
        assert np.array_equal(luts[ch], want_luts)
    one = K.reference(grey[:, :, None], 2.0, (4, 4))
    assert one.shape == (45, 52, 1) and np.array_equal(one[:, :, 0], want)


def test_pil_images_are_taken_as_their_arrays():
    from PIL import Image
    grey = random_image((40, 44), 34)
    assert np.array_equal(K.reference(Image.fromarray(grey, "L"), 2.0, (4, 4)),
                          K.reference(grey, 2.0, (4, 4)))
    rgb = random_image((40, 44, 3), 35)
    assert np.array_equal(K.Clahe(3.0, (2, 4))(Image.fromarray(rgb, "RGB")),
                          K.reference(rgb, 3.0, (2, 4)))


def test_the_gpu_cases_take_both_residual_paths():
    """random_224 hands its residual out in steps > 1, smooth_224 has res > 128 (step 1)."""
    for name, want_step_one in (("random_224", False), ("smooth_224", True)):
        img, clip_limit, tiles, _, _ = case(name)
        tw, th, clip, _ = K.geometry(*img.shape, clip_limit, tiles)
        hist = K.tile_histograms(img, tiles, tw, th)
        res = np.maximum(hist - clip, 0).sum(-1) % 256
        if want_step_one:
            assert (res > 128).any()
        else:
            assert ((res > 0) & (256 // np.maximum(res, 1) > 1)).any()


# ----------------------------------------------------------------------------- extension
def test_extension_pads_both_axes_when_one_does_not_divide():
    # H = 30 is no multiple of 8, W = 32 is: both grow, W by a whole 8
    assert K.geometry(30, 32, 2.0, (8, 8))[:2] == (5, 4)
    assert K.geometry(32, 32, 2.0, (8, 8))[:2] == (4, 4)
    assert K.geometry(29, 37, 2.0, (4, 3))[:2] == (10, 10)
    for shape, tiles in (((30, 32), (8, 8)), ((29, 37), (4, 3))):
        img = random_image(shape, 36)
        tw, th, clip, scale = K.geometry(*shape, 2.0, tiles)
        parts = _tiles_of(img, tiles, tw, th)
        _, luts = K.reference(img, 2.0, tiles, return_luts=True)
        for j in range(tiles[1]):
            for i in range(tiles[0]):
                h = serial_redistribute(np.bincount(parts[j][i].ravel(), minlength=256), clip)
                lut = np.rint(np.cumsum(h).astype(np.float32) * scale)
                assert np.array_equal(luts[j, i], lut.astype(np.uint8)), (shape, j, i)
    # the last tile column of [30, 32] lies wholly in the reflected border
    img = random_image((30, 32), 36)
    ext = np.pad(img, ((0, 2), (0, 8)), mode="reflect")
    assert np.array_equal(ext[:30, 35:40], img[:, [27, 26, 25, 24, 23]])


def test_interpolation_on_a_small_image_by_hand():
    """Step 4 pixel by pixel with Python floats rounded through float32 after every operation."""
    f32 = np.float32
    img = random_image((12, 10), 37)
    tiles = (2, 3)
    out, luts = K.reference(img, 2.0, tiles, return_luts=True)
    tw, th = K.geometry(12, 10, 2.0, tiles)[:2]
    for y in range(12):
        fy = f32(f32(y) * (f32(1) / f32(th))) - f32(0.5)
        y1 = int(np.floor(fy))
        ya = f32(fy - f32(y1))
        ya1 = f32(f32(1) - ya)
        for x in range(10):
            fx = f32(f32(x) * (f32(1) / f32(tw))) - f32(0.5)
            x1 = int(np.floor(fx))
            xa = f32(fx - f32(x1))
            xa1 = f32(f32(1) - xa)
            r1, r2 = max(y1, 0), min(y1 + 1, tiles[1] - 1)
            c1, c2 = max(x1, 0), min(x1 + 1, tiles[0] - 1)
            v = img[y, x]
            top = f32(f32(f32(luts[r1, c1, v]) * xa1) + f32(f32(luts[r1, c2, v]) * xa))
            bot = f32(f32(f32(luts[r2, c1, v]) * xa1) + f32(f32(luts[r2, c2, v]) * xa))
            r = f32(f32(top * ya1) + f32(bot * ya))
            assert out[y, x] == min(max(int(np.rint(r)), 0), 255), (y, x)


# ----------------------------------------------------------------------------- plan
def test_plan_descriptors_of_a_mixed_batch():
    arrays = [K.as_planes(a) for a in mixed_batch()]
    c = mmdx.Clahe(2.0, (4, 2))
    descs, total, lut_bytes = K.plan(arrays, c)
    assert descs.dtype == K.DESC and K.DESC.itemsize == 64
    assert K.DESC.names == ("src_off", "dst_off", "lut_off", "w", "h", "c", "tiles_x", "tiles_y",
                            "tile_w", "tile_h", "clip", "lut_scale")
    off = lut_off = 0
    for d, a in zip(descs, arrays):
        h, w, ch = a.shape
        if w % 4 == 0 and h % 2 == 0:
            w_ext, h_ext = w, h
        else:
            w_ext, h_ext = w + 4 - w % 4, h + 2 - h % 2
        tw, th = w_ext // 4, h_ext // 2
        assert (d["src_off"], d["dst_off"], d["lut_off"]) == (off, off, lut_off)
        assert (d["w"], d["h"], d["c"]) == (w, h, ch)
        assert (d["tiles_x"], d["tiles_y"], d["tile_w"], d["tile_h"]) == (4, 2, tw, th)
        assert d["clip"] == max(int(2.0 * tw * th / 256), 1)
        assert d["lut_scale"] == np.float32(255) / np.float32(tw * th)
        assert d["lut_scale"].dtype == np.float32
        off += a.size
        lut_off += ch * 8 * 256
    assert (total, lut_bytes) == (off, lut_off)
    # (29, 37): H does not divide by 2 and W not by 4 -> 30 x 40
    assert (descs[1]["tile_w"], descs[1]["tile_h"]) == (10, 15)
    assert K.plan(arrays[:1], mmdx.Clahe(0, (2, 2)))[0][0]["clip"] == 0
    assert K.plan(arrays[:1], mmdx.Clahe(-1.0, (2, 2)))[0][0]["clip"] == 0
    # a clip of the area or more clips nothing: it is capped there (an int32 for any clip_limit)
    assert K.plan(arrays[:1], mmdx.Clahe(1e300, (2, 2)))[0][0]["clip"] == 64


def test_plan_matches_the_c_struct():
    from mmdx import _lib as L
    assert L.lib().mmdx_clahe_desc_size() == K.DESC.itemsize


# ----------------------------------------------------------------------------- config
def test_config_round_trips_through_json_and_the_bundle_config():
    from mmdx.inference_pipeline import bundle_config
    c = mmdx.Clahe(clip_limit=3, tiles=(np.int64(4), 6))
    cfg = c.config()
    assert cfg == {"clip_limit": 3.0, "tiles": [4, 6]}
    assert type(cfg["clip_limit"]) is float and all(type(t) is int for t in cfg["tiles"])
    back = mmdx.Clahe.from_config(json.loads(json.dumps(cfg)))
    assert back == c and back.tiles == (4, 6) and back.config() == cfg
    assert mmdx.Clahe().config() == {"clip_limit": 2.0, "tiles": [8, 8]}
    mods = [types.SimpleNamespace() for _ in range(3)]
    whole = bundle_config(*mods, artifacts={"thresholds": [0.5] * 13, "clahe": cfg})
    stored = json.loads(json.dumps(whole))["artifacts"]["clahe"]
    assert stored == cfg and mmdx.Clahe.from_config(stored) == c
    assert "artifacts" not in bundle_config(*mods)
    with pytest.raises(ValueError):
        mmdx.Clahe.from_config({"clip_limit": 2.0})
    with pytest.raises(TypeError):
        mmdx.Clahe.from_config([2.0, (8, 8)])


def test_arguments_default_to_off():
    import inspect
    from mmdx.data import LocalCXRBatches
    from mmdx.preprocess import preprocess_batch
    from mmdx.training_driver import training_tests
    for fn in (preprocess_batch, LocalCXRBatches.__init__, training_tests):
        assert inspect.signature(fn).parameters["clahe"].default is None
    assert mmdx.Clahe is K.Clahe


# ----------------------------------------------------------------------------- limits
def test_limits_raise_the_documented_errors():
    img = random_image((64, 64), 38)
    with pytest.raises(TypeError):
        K.reference(img.astype(np.uint16), 2.0, (8, 8))
    with pytest.raises(TypeError):
        K.reference(img.astype(np.float32), 2.0, (8, 8))
    with pytest.raises(ValueError):
        K.reference(random_image((64, 64, 2), 39), 2.0, (8, 8))
    with pytest.raises(ValueError):
        K.reference(random_image((64, 64, 4), 39), 2.0, (8, 8))
    with pytest.raises(ValueError):
        K.reference(random_image((4, 64, 64, 3), 39), 2.0, (8, 8))
    for tiles in ((0, 8), (8, 17), (-1, 2)):
        with pytest.raises(ValueError):
            mmdx.Clahe(2.0, tiles)
    for tiles in ((8.0, 8), 8, (8, 8, 8), ("8", 8), (True, 8)):
        with pytest.raises(TypeError):
            mmdx.Clahe(2.0, tiles)
    for clip in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            mmdx.Clahe(clip)
    for clip in ("2", None, True):
        with pytest.raises(TypeError):
            mmdx.Clahe(clip)
    c = mmdx.Clahe()
    c.tiles = (32, 32)          # check() re-validates a changed object
    with pytest.raises(ValueError):
        c.check()
    with pytest.raises(ValueError):
        c.config()
    # W >= 2 tx and H >= 2 ty
    assert K.reference(random_image((16, 16), 40), 2.0, (8, 8)).shape == (16, 16)
    with pytest.raises(ValueError):
        K.reference(random_image((16, 15), 40), 2.0, (8, 8))
    with pytest.raises(ValueError):
        K.reference(random_image((15, 16), 40), 2.0, (8, 8))
    with pytest.raises(ValueError):
        K.plan([K.as_planes(random_image((31, 64), 40))], mmdx.Clahe(2.0, (8, 16)))
    # tile area <= 2^24 and sides <= 65535, from the shape alone
    assert K.geometry(4096, 4096, 2.0, (1, 1))[:2] == (4096, 4096)
    with pytest.raises(ValueError):
        K.geometry(4096, 4100, 2.0, (1, 1))
    with pytest.raises(ValueError):
        K.geometry(8, 65536, 2.0, (2, 2))
    with pytest.raises(ValueError):
        K.plan([], mmdx.Clahe())
    with pytest.raises(TypeError):
        K.plan([K.as_planes(img)], {"clip_limit": 2.0, "tiles": [8, 8]})
    with pytest.raises(TypeError):
        K.plan([img.astype(np.int32)[:, :, None]], mmdx.Clahe())
    from PIL import Image
    with pytest.raises(ValueError):
        K.reference(Image.fromarray(img, "L").convert("RGBA"), 2.0, (8, 8))


def test_entry_points_reject_bad_arguments_without_a_device():
    """functional.clahe and preprocess_batch raise the limits before they touch the GPU."""
    import mmdx.functional as F
    with pytest.raises(ValueError):
        F.clahe([random_image((15, 16), 41)], tiles=(8, 8))
    with pytest.raises(TypeError):
        F.clahe([random_image((32, 32), 41).astype(np.int16)])
    with pytest.raises(ValueError):
        F.clahe([random_image((32, 32), 41)], clip_limit=float("nan"))
    with pytest.raises(TypeError):
        F.clahe(random_image((32, 32), 41))
    with pytest.raises(TypeError):
        mmdx.preprocess_batch([random_image((300, 300), 41)], clahe=(2.0, (8, 8)))
    from mmdx.training_driver import training_tests
    with pytest.raises(TypeError):
        training_tests(clahe={"clip_limit": 2.0, "tiles": [8, 8]})


def test_smooth_and_two_level_cases_are_what_they_say():
    s = smooth_image()
    assert s.shape == (224, 224) and s.min() >= 28 and s.max() <= 228
    assert sorted(np.unique(two_level_image()).tolist()) == [40, 200]
