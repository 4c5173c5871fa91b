"""CPU: mmdx.window's numpy `reference` (the definition the kernels are held to), the ranks,
the descriptor table, the limits, the setting's config and its way through the bundle, the
CPU-device inference() path and the case index.  No GPU."""
import inspect
import json
import math

import numpy as np
import pytest
import torch
from PIL import Image

import mmdx
from mmdx import data as D
from mmdx import window as W

from window_cases import IMAGES, SHAPES, boundary, expected, image, mixed_batch, windows

TEXT = "44 year old female PA view , hypertension , cough"


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("name", sorted(n for n in IMAGES if not n.endswith("_big")))
def test_order_statistics_are_the_sorted_pixels(name):
    img = image(name)
    s = np.sort(img.ravel())
    for low, high in ((0.5, 99.5), (0, 100), (25, 75), (10, 10.001), (99.9, 100)):
        k_lo, k_hi = W.ranks(img.size, low, high)
        _, (lo, hi) = W.reference(img, W.Window(low=low, high=high), return_window=True)
        assert lo == int(s[k_lo])
        assert hi == (int(s[k_hi]) if s[k_hi] != s[k_lo] else lo + 1)
        assert isinstance(lo, int) and isinstance(hi, int)


def test_ranks():
    assert W.ranks(1, 0, 100) == (0, 0)
    assert W.ranks(1, 0.5, 99.5) == (0, 0)
    assert W.ranks(10, 0, 100) == (0, 9)           # high = 100 is the maximum, not index n
    assert W.ranks(200, 0.5, 99.5) == (1, 199)
    assert W.ranks(4, 25, 75) == (1, 3)
    assert W.ranks(1 << 30, 0.5, 99.5) == (math.floor(0.5 * (1 << 30) / 100),
                                           math.floor(99.5 * (1 << 30) / 100))
    with pytest.raises(ValueError):
        W.ranks(0, 0, 100)


def test_boundary_image_takes_the_next_populated_level():
    for shape in ((2, 2), (64, 64)):
        _, (lo, hi) = W.reference(boundary(shape), W.Window(low=25, high=75),
                                  return_window=True)
        assert (lo, hi) == (2000, 60000)
    _, (lo, hi) = W.reference(boundary((64, 64)), W.Window(low=24.99, high=74.99),
                              return_window=True)
    assert (lo, hi) == (100, 2000)


@pytest.mark.parametrize("value", [0, 40000, 65535])
def test_flat_image_rule(value):
    img = np.full((5, 9), value, np.uint16)
    out, (lo, hi) = W.reference(img, W.Window(), return_window=True)
    assert (lo, hi) == (value, value + 1)
    assert out.dtype == np.uint8 and out.shape == (5, 9) and (out == 0).all()
    assert (W.reference(img, W.Window(invert=True)) == 255).all()


def test_ties_round_half_to_even():
    ramp = np.arange(512, dtype=np.uint16)[None, :]
    w = W.Window("fixed", lo=0, hi=510)
    assert W.scale_of(0, 510) == np.float32(0.5)
    out = W.reference(ramp, w)
    assert out[0, :8].tolist() == [0, 0, 1, 2, 2, 2, 3, 4]
    assert out[0, -3:].tolist() == [254, 255, 255]
    # the same through min-max: lo = 0, hi = 511 is not a tie case, 0 .. 510 is
    out2, win = W.reference(ramp[:, :511], W.Window(low=0, high=100), return_window=True)
    assert win == (0, 510) and np.array_equal(out2, out[:, :511])


def test_mapping_against_float64():
    """The fp32 steps against the exact value: (v - lo) is exact, so the result is within the
    rounding of one division and one multiply of 255 (v - lo) / (hi - lo)."""
    img = image("uniform_37x53")
    for w in (W.Window("fixed", lo=1023.5, hi=3071.5), W.Window("fixed", lo=-1000.5, hi=70000.0),
              W.Window(low=0, high=100)):
        out, (lo, hi) = W.reference(img, w, return_window=True)
        exact = np.clip((img.astype(np.float64) - lo) * 255.0 / (hi - lo), 0, 255)
        assert np.abs(out - exact).max() <= 0.5 + 255 * 2.0 ** -22


def test_from_center_width_is_dicoms_linear_voi():
    """DICOM PS3.3 C.11.2.1.2.1 in float64: y = ((x - (c - 0.5)) / (w - 1) + 0.5) * 255 between
    the two clamps at x <= c - 0.5 - (w - 1) / 2 and x > c - 0.5 + (w - 1) / 2."""
    x = np.arange(0, 4096, dtype=np.uint16)[None, :]
    for c, w in ((2048, 4096), (1800, 601), (600, 2), (40, 400), (-20, 301)):
        win = W.Window.from_center_width(c, w)
        assert win.mode == "fixed" and win.lo == c - 0.5 - (w - 1) / 2 and win.hi == win.lo + w - 1
        xf = x.astype(np.float64)
        y = ((xf - (c - 0.5)) / (w - 1) + 0.5) * 255.0
        y = np.where(xf <= c - 0.5 - (w - 1) / 2, 0.0, np.where(xf > c - 0.5 + (w - 1) / 2,
                                                                 255.0, y))
        got = W.reference(x, win).astype(np.float64)
        assert np.abs(got - y).max() <= 0.5 + 255 * 2.0 ** -22
    with pytest.raises(ValueError):
        W.Window.from_center_width(100, 1)
    with pytest.raises(TypeError):
        W.Window.from_center_width(100.5, 10)
    with pytest.raises(TypeError):
        W.Window.from_center_width(100, 10.0)


def test_invert_is_255_minus_the_plain_result():
    for name in ("gauss12_37x53", "uniform_3x5", "two_valued_3x5"):
        for wname in ("percentile", "minmax", "fixed_half", "fixed_wide"):
            plain, win = expected(name, wname)
            inv, win_i = expected(name, wname + "_inv")
            assert win == win_i and np.array_equal(inv, 255 - plain)


def test_input_forms():
    img = image("gauss12_37x53")
    w = W.Window()
    want = W.reference(img, w)
    assert np.array_equal(W.reference(img[:, :, None], w), want)
    pil = Image.fromarray(np.array(img))
    assert pil.mode == "I;16"
    assert np.array_equal(W.reference(pil, w), want) and np.array_equal(w(pil), want)


def test_a_16_bit_png_opens_as_i16(tmp_path):
    img = image("gauss12_37x53")
    Image.fromarray(np.array(img)).save(tmp_path / "a.png")
    back = D.open_image(str(tmp_path), "a.png")
    assert back.mode == "I;16" and np.array_equal(W.as_plane(back), img)


# ----------------------------------------------------------------------------- limits
def test_limits_raise_the_documented_errors():
    for kw in (dict(low=-1), dict(high=100.5), dict(low=50, high=50), dict(low=60, high=40),
               dict(low=float("nan")), dict(high=float("inf")), dict(mode="sigmoid"),
               dict(mode="fixed"), dict(mode="fixed", lo=0), dict(mode="fixed", lo=5, hi=5),
               dict(mode="fixed", lo=0.25, hi=10), dict(mode="fixed", lo=0, hi=10.1),
               dict(mode="fixed", lo=-65536.5, hi=10), dict(mode="fixed", lo=0, hi=131072.5),
               dict(mode="fixed", lo=float("nan"), hi=10), dict(mode="fixed", lo=0,
                                                                 hi=float("inf")),
               dict(lo=0, hi=10)):
        with pytest.raises(ValueError):
            W.Window(**kw)
    for kw in (dict(mode=1), dict(low="1"), dict(high=None), dict(low=True),
               dict(mode="fixed", lo="0", hi=10), dict(invert=1), dict(invert="no")):
        with pytest.raises(TypeError):
            W.Window(**kw)
    assert W.Window("fixed", lo=-65536, hi=131072).check()
    w = W.Window()
    img = image("uniform_3x5")
    for bad in (img.astype(np.uint8), img.astype(np.int16), img.astype(np.int32),
                img.astype(np.float32), Image.fromarray(img.astype(np.uint8), "L"),
                Image.fromarray(img.astype(np.int32), "I")):
        with pytest.raises(TypeError):
            W.reference(bad, w)
    for bad in (np.zeros((4, 4, 3), np.uint16), np.zeros((4,), np.uint16),
                np.zeros((0, 4), np.uint16), np.zeros((2, 2, 1, 1), np.uint16),
                np.broadcast_to(np.uint16(0), (65536, 1)), np.broadcast_to(np.uint16(0), (1, 65536)),
                np.broadcast_to(np.uint16(0), (40000, 40000))):
        with pytest.raises(ValueError):
            W.as_plane(bad)
    with pytest.raises(TypeError):
        W.reference(img, {"mode": "percentile"})
    with pytest.raises(ValueError):
        W.plan([], w)
    with pytest.raises(TypeError):
        W.plan([img.astype(np.uint8)], w)
    with pytest.raises(ValueError):
        W.plan([img[:, :, None]], w)
    with pytest.raises(TypeError):
        W.plan([img], (0.5, 99.5))


def test_entry_points_reject_bad_arguments_without_a_device():
    """functional.window16 and preprocess_batch raise the limits before they touch the GPU."""
    import mmdx.functional as F
    from mmdx.training_driver import training_tests
    img = image("uniform_37x53")
    with pytest.raises(TypeError):
        F.window16([img], (0.5, 99.5))
    with pytest.raises(TypeError):
        F.window16(img, W.Window())
    with pytest.raises(TypeError):
        F.window16([img.astype(np.uint8)], W.Window())
    with pytest.raises(ValueError):
        F.window16([np.zeros((4, 4, 3), np.uint16)], W.Window())
    with pytest.raises(ValueError):
        F.window16([], W.Window())
    with pytest.raises(TypeError):
        mmdx.preprocess_batch([img], window={"mode": "percentile"})
    with pytest.raises(TypeError):
        training_tests(window={"mode": "percentile"})
    with pytest.raises(TypeError):
        D.LocalCXRBatches(None, "", window=(0.5, 99.5))


def test_arguments_default_to_off():
    from mmdx.training_driver import training_tests
    for fn in (mmdx.preprocess_batch, D.LocalCXRBatches.__init__, training_tests):
        assert inspect.signature(fn).parameters["window"].default is None
    assert inspect.signature(mmdx.CaseIndex.from_vectors).parameters["window"].default is None
    assert mmdx.Window is W.Window


# ----------------------------------------------------------------------------- descriptors
def test_plan_descriptors_of_a_mixed_batch():
    planes = mixed_batch()
    descs, src, dst = W.plan(planes, W.Window(low=1, high=99, invert=True))
    assert len(descs) == len(planes) and dst == sum(a.size for a in planes) and src % 16 == 0
    so = do = 0
    for d, a in zip(descs, planes):
        assert (d["src_off"], d["dst_off"]) == (so, do) and so % 16 == 0
        assert (d["h"], d["w"]) == a.shape and d["mode"] == 0 and d["invert"] == 1
        assert (d["k_lo"], d["k_hi"]) == W.ranks(a.size, 1, 99)
        so += -(-2 * a.size // 16) * 16
        do += a.size
    assert so == src
    # the destination is the packed layout of the 8-bit plans for (H, W, 1) arrays
    as8 = [np.zeros(a.shape + (1,), np.uint8) for a in planes]
    cl, total, _ = mmdx.clahe.plan([a for a in as8 if min(a.shape[:2]) >= 2],
                                   mmdx.Clahe(2.0, (1, 1)))
    assert total == sum(a.size for a in as8 if min(a.shape[:2]) >= 2)
    host = np.zeros(src, np.uint8)
    W.pack(planes, descs, host)
    for d, a in zip(descs, planes):
        o = int(d["src_off"])
        assert np.array_equal(host[o:o + 2 * a.size].view(np.uint16), a.ravel())
    fx, _, _ = W.plan(planes[:2], W.Window("fixed", lo=-0.5, hi=4095.5))
    assert fx[0]["mode"] == 1 and fx[0]["lo"] == -0.5 and fx[0]["hi"] == 4095.5
    assert fx[0]["scale"] == np.float32(255) / np.float32(4096) and fx[0]["invert"] == 0


def test_plan_matches_the_c_struct_and_the_workspace_query_is_host_only():
    lib = mmdx._lib.lib()
    assert lib.mmdx_window_desc_size() == W.DESC.itemsize
    assert lib.mmdx_window_workspace_size(1) == 65536 * 4
    assert lib.mmdx_window_workspace_size(128) == 128 * 65536 * 4
    assert lib.mmdx_window_workspace_size(0) == 0 == lib.mmdx_window_workspace_size(65536)


def test_the_gpu_cases_are_what_they_say():
    assert [image(f"uniform_{h}x{w}").shape for h, w in SHAPES] == SHAPES
    g = image("gauss12_big")
    assert g.max() < 4096 and 1700 < g.mean() < 1900 and len(np.unique(g)) > 500
    r = image("radiograph_big")
    assert (r[:, :256] == 4095).mean() > 0.8 and (r[-128:] == 0).all()
    assert image("with65535_37x53").max() == 65535 and image("with65535_37x53").min() == 0
    assert expected("with65535_257x129", "minmax")[1] == (0, 65535)
    assert set(np.unique(image("two_valued_257x129"))) == {0, 65535}
    assert expected("two_valued_257x129", "percentile")[1] == (0, 65535)
    assert expected("all65535_37x53", "minmax")[1] == (65535, 65536)


# ----------------------------------------------------------------------------- config, bundle
def test_config_round_trips_through_json_and_the_bundle_config():
    from mmdx.inference_pipeline import bundle_config
    for w in list(windows().values()) + [W.Window.from_center_width(1800, 601),
                                         W.Window(low=np.float32(1), high=np.int64(99))]:
        cfg = w.config()
        back = W.Window.from_config(json.loads(json.dumps(cfg)))
        assert back == w and back.config() == cfg and repr(back) == repr(w)
        assert hash(back) == hash(w)
    assert W.Window().config() == {"mode": "percentile", "low": 0.5, "high": 99.5,
                                   "invert": False}
    assert W.Window("fixed", lo=0, hi=4095, invert=True).config() == \
        {"mode": "fixed", "lo": 0.0, "hi": 4095.0, "invert": True}
    assert W.Window() != W.Window(invert=True) and W.Window() != "percentile"
    assert repr(W.Window()) == "Window(mode='percentile', low=0.5, high=99.5, invert=False)"
    w = W.Window()
    assert W.Window.from_config(w) is w
    mods = (torch.nn.Linear(2, 2),) * 3
    whole = bundle_config(*mods, artifacts={"thresholds": [0.5] * 13, "window": w.config()})
    assert W.Window.from_config(json.loads(json.dumps(whole))["artifacts"]["window"]) == w
    with pytest.raises(ValueError):
        W.Window.from_config({"low": 1, "high": 99})
    with pytest.raises(ValueError):
        W.Window.from_config({"mode": "fixed", "lo": 1})
    with pytest.raises(TypeError):
        W.Window.from_config(["percentile", 0.5, 99.5])
    w.low = 200
    with pytest.raises(ValueError):
        w.config()


@pytest.fixture(scope="module")
def bundles(tmp_path_factory):
    """One small model saved twice: with artifacts["window"] and without."""
    from mmdx.inference_pipeline import load_model_bundle, save_model_bundle
    torch.manual_seed(0)
    img = mmdx.ImageEncoderCNN("resnet18", 1024, 13)
    txt = mmdx.TextEncoderTransformer("embed-mean", 512, 13)
    fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13)
    w = W.Window(low=1, high=99, invert=True)
    arts = {"class_names": list(mmdx.DISEASES), "thresholds": [0.5] * 13}
    d = tmp_path_factory.mktemp("window_bundles")
    p_w = save_model_bundle(fus, img, txt, str(d / "w"), timestamped_copy=False,
                            artifacts=dict(arts, window=w.config()))
    p_raw = save_model_bundle(fus, img, txt, str(d / "raw"), timestamped_copy=False,
                              artifacts=arts)
    return (w, load_model_bundle(p_w, device="cpu", with_report_head=False),
            load_model_bundle(p_raw, device="cpu", with_report_head=False))


def test_bundle_artifact_round_trip(bundles):
    w, b_w, b_raw = bundles
    assert b_w["window"] == w.config() and W.Window.from_config(b_w["window"]) == w
    assert b_raw["window"] is None and b_raw["clahe"] is None and b_w["clahe"] is None


def test_cpu_inference_windows_with_the_reference(bundles, monkeypatch):
    """On a CPU device inference() windows with mmdx.window.reference before the transform: the
    transform receives exactly those bytes.  (The towers themselves are GPU-only: the run ends
    at the image tower with its RuntimeError, after the transform.)"""
    from mmdx import inference_pipeline as IP
    w, b_w, b_raw = bundles
    img16 = np.array(image("gauss12_257x129"))
    seen = []
    real = IP.image_transfom_into_tensor

    def spy(pil):
        seen.append(np.asarray(pil).copy())
        return real(pil)

    monkeypatch.setattr(IP, "image_transfom_into_tensor", spy)
    for form in (img16, Image.fromarray(img16)):
        with pytest.raises(RuntimeError, match="GPU"):
            IP.inference(b_w, form, TEXT, device="cpu")
        assert seen[-1].dtype == np.uint8 and np.array_equal(seen[-1], W.reference(img16, w))
    # with CLAHE in the bundle too: window first, then equalisation
    c = mmdx.Clahe(2.0, (4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        IP.inference(dict(b_w, clahe=c.config()), img16, TEXT, device="cpu")
    assert np.array_equal(seen[-1], c(W.reference(img16, w)))
    # an 8-bit image to a bundle that carries a window: refused, and saying why
    n = len(seen)
    for bad in (Image.fromarray(W.reference(img16, w)), W.reference(img16, w),
                Image.fromarray(W.reference(img16, w)).convert("RGB")):
        with pytest.raises(ValueError, match="16-bit"):
            IP.inference(b_w, bad, TEXT, device="cpu")
    assert len(seen) == n
    # a bundle without the key takes the 8-bit image as before
    pil8 = Image.fromarray(W.reference(img16, w))
    with pytest.raises(RuntimeError, match="GPU"):
        IP.inference(b_raw, pil8, TEXT, device="cpu")
    assert np.array_equal(seen[-1], np.asarray(pil8))
    no_key = {k: v for k, v in b_raw.items() if k != "window"}
    with pytest.raises(RuntimeError, match="GPU"):
        IP.inference(no_key, pil8, TEXT, device="cpu")
    assert np.array_equal(seen[-1], np.asarray(pil8))


# ----------------------------------------------------------------------------- case index
def test_index_meta_carries_the_window_and_a_mismatch_is_refused(bundles, tmp_path):
    from mmdx.inference_pipeline import bundle_fingerprint, inference_similar
    w, b_w, b_raw = bundles
    g = torch.Generator().manual_seed(1)
    v, y = torch.randn(4, 1024, generator=g), torch.zeros(4, 13)
    keys = [f"k{i}" for i in range(4)]
    fp = bundle_fingerprint(b_w)
    plain = mmdx.CaseIndex.from_vectors(v, y, keys, fingerprint=fp)
    assert "window" not in plain.meta           # an index of 8-bit images is what it was
    idx = mmdx.CaseIndex.from_vectors(v, y, keys, fingerprint=fp, window=w.config())
    assert idx.meta["window"] == w.config()
    back = mmdx.CaseIndex.load(idx.save(tmp_path / "case_index.pt"), device="cpu")
    assert back.meta == idx.meta
    old = mmdx.CaseIndex.load(plain.save(tmp_path / "old.pt"), device="cpu")
    assert old.meta.get("window") is None
    img16 = np.array(image("gauss12_37x53"))
    other = W.Window(low=2, high=98).config()
    for index, bundle in ((plain, b_w), (old, b_w), (idx, b_raw), (idx, dict(b_w, window=other))):
        with pytest.raises(ValueError, match="window"):
            inference_similar(bundle, img16, TEXT, index, device="cpu")
    # matching windows pass that check (the run then ends at the GPU-only image tower)
    with pytest.raises(RuntimeError, match="GPU"):
        inference_similar(b_w, np.zeros((300, 300), np.uint16), TEXT, idx, device="cpu")
