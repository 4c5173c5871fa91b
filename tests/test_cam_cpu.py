"""CPU: the host half of the Grad-CAM feature (mmdx.explain: cam_to_image, overlay, class
selection), the argument checks of the two CAM entry points (they precede any HIP call, so they
run without a GPU), the wrappers' refusal of CPU tensors, and the ViT refusal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-modal-medical-imaging-and-report-ml-diagnosis-system_amd")


# ----------------------------------------------------------------------------- C ABI checks
@pytest.fixture(scope="module")
def lib():
    import mmdx
    if not os.path.exists(mmdx._lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    return mmdx._lib.lib()


def _rejected(lib, rc, needle):
    assert rc != 0
    msg = lib.mmdx_last_error().decode()
    assert needle in msg, msg


def test_cam_fwd_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(256 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    f = lib.mmdx_cam_fwd
    # (dtype, fmap, alpha, B, HW, K, C, raw, stream)
    _rejected(lib, f(1, None, p, 1, 4, 8, 2, p, None), "null")
    _rejected(lib, f(1, p, None, 1, 4, 8, 2, p, None), "null")
    _rejected(lib, f(1, p, p, 1, 4, 8, 2, None, None), "null")
    _rejected(lib, f(3, p, p, 1, 4, 8, 2, p, None), "dtype = 3")
    _rejected(lib, f(1, p, p, 0, 4, 8, 2, p, None), "B = 0")
    _rejected(lib, f(1, p, p, 1, 0, 8, 2, p, None), "HW = 0")
    _rejected(lib, f(1, p, p, 1, 4, 0, 2, p, None), "K = 0")
    _rejected(lib, f(1, p, p, 1, 4, 8, 0, p, None), "C = 0")
    _rejected(lib, f(1, p, p, -2, 4, 8, 2, p, None), "B = -2")
    _rejected(lib, f(1, p, p, 1, 4, 12, 2, p, None), "K = 12")
    _rejected(lib, f(0, p, p, 1, 4, 2052, 2, p, None), "K = 2052")
    _rejected(lib, f(1, p, p, 1, 4, 8, 65, p, None), "C = 65")
    _rejected(lib, f(1, p, p, 1, 1025, 8, 2, p, None), "HW = 1025")
    _rejected(lib, f(1, p + 2, p, 1, 4, 8, 2, p, None), "aligned")


def test_cam_resize_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(256 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    f = lib.mmdx_cam_resize
    # (raw, BC, H, W, Ho, Wo, normalize, out, stream)
    _rejected(lib, f(None, 1, 2, 2, 4, 4, 1, p, None), "null")
    _rejected(lib, f(p, 1, 2, 2, 4, 4, 1, None, None), "null")
    _rejected(lib, f(p, 0, 2, 2, 4, 4, 1, p, None), "BC = 0")
    _rejected(lib, f(p, 1, 0, 2, 4, 4, 1, p, None), "H = 0")
    _rejected(lib, f(p, 1, 2, 0, 4, 4, 1, p, None), "W = 0")
    _rejected(lib, f(p, 1, 2, 2, 0, 4, 1, p, None), "Ho = 0")
    _rejected(lib, f(p, 1, 2, 2, 4, -1, 1, p, None), "Wo = -1")
    _rejected(lib, f(p, 1, 33, 32, 4, 4, 1, p, None), "H * W = 1056")
    _rejected(lib, f(p, 1, 1025, 1, 4, 4, 0, p, None), "H * W = 1025")
    _rejected(lib, f(p, 1, 2, 2, 4097, 4, 1, p, None), "Ho = 4097")
    _rejected(lib, f(p, 1, 2, 2, 4, 4097, 1, p, None), "Wo = 4097")


def test_functional_wrappers_refuse_cpu_tensors():
    import torch
    import mmdx.functional as F
    with pytest.raises(RuntimeError, match="GPU"):
        F.cam_raw(torch.zeros(1, 2, 2, 8), torch.zeros(1, 3, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        F.cam_resize(torch.zeros(1, 3, 2, 2), (8, 8))


# ----------------------------------------------------------------------------- cam_to_image
def _crop_box(w, h):
    """The centre-crop rectangle in original pixels, from the preprocessing's own definition:
    shorter side -> 256, a centred 224 window, so 224 / 256 of the shorter side, centred."""
    side = 224.0 / 256.0 * min(w, h)
    return (w - side) / 2.0, (h - side) / 2.0, (w + side) / 2.0, (h + side) / 2.0


@pytest.mark.parametrize("size", [(512, 512), (300, 500), (500, 300)])
def test_cam_to_image_covers_exactly_the_crop(size):
    from mmdx.explain import cam_to_image
    w, h = size
    m = cam_to_image(np.ones((224, 224), np.float32), size)
    assert m.shape == (h, w) and m.dtype == np.float32
    ys, xs = np.nonzero(m)
    x0, y0, x1, y1 = _crop_box(w, h)
    # a filled rectangle of ones ...
    assert len(ys) == (ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1)
    np.testing.assert_allclose(m[ys, xs], 1.0, atol=1e-6)
    # ... whose edges are the crop's, to the pixel (the resized long side is truncated to an
    # integer by the preprocessing, which moves an edge by less than one original pixel)
    assert abs(xs.min() - x0) <= 1 and abs(xs.max() + 1 - x1) <= 1
    assert abs(ys.min() - y0) <= 1 and abs(ys.max() + 1 - y1) <= 1


def test_cam_to_image_512_box_is_exact():
    from mmdx.explain import cam_to_image
    m = cam_to_image(np.ones((224, 224), np.float32), (512, 512))
    want = np.zeros((512, 512), np.float32)
    want[32:480, 32:480] = 1.0
    np.testing.assert_allclose(m, want, atol=1e-6)


def test_cam_to_image_keeps_orientation():
    from mmdx.explain import cam_to_image
    cam = np.zeros((224, 224), np.float32)
    cam[:112, 112:] = 1.0            # top-right quadrant
    m = cam_to_image(cam, (640, 480))
    assert m.shape == (480, 640)
    assert m[120:230, 330:500].min() > 0.99           # top-right of the centre crop
    assert m[250:, :].max() < 0.01                    # nothing in the lower half
    assert m[:, :300].max() < 0.01                    # nothing in the left half
    with pytest.raises(ValueError):
        cam_to_image(np.ones((7, 7), np.float32), (640, 480))


# ----------------------------------------------------------------------------- overlay
def test_overlay_size_mode_dtype_and_zero_map_identity():
    from mmdx.explain import overlay
    rng = np.random.default_rng(0)
    rgb = Image.fromarray(rng.integers(0, 256, (40, 60, 3), dtype=np.uint8))
    out = overlay(rgb, np.zeros((40, 60), np.float32))
    assert out.size == (60, 40) and out.mode == "RGB"
    a = np.asarray(out)
    assert a.dtype == np.uint8 and np.array_equal(a, np.asarray(rgb))
    gray = rgb.convert("L")
    out = overlay(gray, np.zeros((40, 60), np.float32))
    assert out.mode == "RGB" and np.array_equal(np.asarray(out), np.asarray(gray.convert("RGB")))


def test_overlay_blends_the_ramp():
    from mmdx.explain import overlay
    img = Image.new("RGB", (4, 2), (100, 100, 100))
    cam = np.zeros((2, 4), np.float32)
    cam[0, 0] = 1.0       # the hot end of the ramp is red
    cam[1, 3] = 0.5       # its middle is green
    a = np.asarray(overlay(img, cam, alpha=0.5)).astype(int)
    assert a[0, 0, 0] > 100 > a[0, 0, 2] and a[0, 0, 0] > a[0, 0, 1]
    assert a[1, 3, 1] > 100 and a[1, 3, 1] > a[1, 3, 0] and a[1, 3, 1] > a[1, 3, 2]
    assert (a[0, 1:] == 100).all()
    with pytest.raises(ValueError):
        overlay(img, np.zeros((4, 2), np.float32))


# ----------------------------------------------------------------------------- selection
def test_select_classes():
    from mmdx.explain import select_classes
    names = ["a", "b", "c", "d"]
    probs = [0.2, 0.9, 0.6, 0.1]
    assert select_classes(probs, [0.5] * 4, names, True) == [1, 2]
    assert select_classes(probs, [0.95] * 4, names, True) == [1]      # none: the top-1
    assert select_classes(probs, [0.5] * 4, names, 3) == [1, 2, 0]
    assert select_classes(probs, [0.5] * 4, names, ["d", "a"]) == [3, 0]
    with pytest.raises(ValueError):
        select_classes(probs, [0.5] * 4, names, ["zz"])
    with pytest.raises(ValueError):
        select_classes(probs, [0.5] * 4, names, 5)
    with pytest.raises(TypeError):
        select_classes(probs, [0.5] * 4, names, 0.5)


def test_inference_signature_gains_explain_off_by_default():
    import inspect
    from mmdx.inference_pipeline import inference
    p = inspect.signature(inference).parameters
    assert list(p) == ["model_bundle", "image_pil", "patient_details", "device", "gen_kwargs",
                       "explain"]
    assert p["explain"].default is None


# ----------------------------------------------------------------------------- ViT
def test_grad_cam_on_a_vit_encoder_is_not_implemented():
    import mmdx
    from mmdx.explain import grad_cam
    enc = mmdx.ImageEncoderCNN("vit_b_16", 1024, 13)
    assert not hasattr(enc.backbone, "forward_features")
    with pytest.raises(NotImplementedError, match="vit_b_16"):
        grad_cam(enc, None, None, None, None, None)
