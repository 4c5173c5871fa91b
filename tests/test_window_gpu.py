"""GPU: the windowing kernels (csrc/window.hip) against mmdx.window.reference, byte for byte,
and the setting's way through preprocess_batch, LocalCXRBatches and inference().  No tolerances
anywhere: counting is integer, the mapping one exact subtraction, one correctly-rounded
division per image and one multiply per pixel."""
import os

import numpy as np
import pytest
import torch

import mmdx
import mmdx.functional as F
from mmdx import window as W

from window_cases import IMAGES, expected, image, mixed_batch, windows

pytestmark = pytest.mark.gpu

TEXT = "44 year old female PA view , hypertension , cough"


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {want.size} differ, first at {bad[0].tolist()}: " \
           f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def _check(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    assert np.array_equal(got, want), f"{what}: {_first_difference(got, want)}"


@pytest.fixture
def span():
    """Fix the chunks per histogram block (MMDX_WINDOW_SPAN) for one test, then put the
    by-size choice back."""
    def set_span(n):
        os.environ["MMDX_WINDOW_SPAN"] = str(n)
        mmdx._lib.reload_config()
    yield set_span
    os.environ.pop("MMDX_WINDOW_SPAN", None)
    mmdx._lib.reload_config()


# ----------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_output_and_window_equal_the_reference(dev, name):
    """Every pixel class and shape under every mode, plain and inverted."""
    img = image(name)
    for wname, w in windows().items():
        want, want_win = expected(name, wname)
        (out,), (win,) = F.window16([img], w, return_window=True, device=dev)
        assert win == want_win, f"{name} {wname}: window {win}, want {want_win}"
        _check(out, want, f"{name} {wname}")


@pytest.mark.parametrize("chunks", [2, 8])
@pytest.mark.parametrize("name", ["all40000_big", "gauss12_big", "radiograph_big",
                                  "uniform_big", "uniform_257x129"])
def test_blocks_that_walk_several_chunks(dev, span, name, chunks):
    """A histogram block that owns more than one 32768-pixel chunk checks its 16-bit counters
    between chunks (the flat image fills one past half its range in every chunk)."""
    span(chunks)
    for wname in ("percentile", "minmax_inv"):
        want, want_win = expected(name, wname)
        (out,), (win,) = F.window16([image(name)], windows()[wname], return_window=True,
                                    device=dev)
        assert win == want_win
        _check(out, want, f"{name} {wname} span {chunks}")


@pytest.mark.parametrize("wname", ["percentile", "quartiles_inv", "minmax", "fixed_half_inv",
                                   "fixed_wide"])
def test_mixed_batch_in_one_call_twice_and_alone(dev, wname):
    """All small shapes in one batch (source padding, every destination alignment); a second
    call on the same workspace gives the same bytes; an image alone equals its slot."""
    w = windows()[wname]
    imgs = mixed_batch()
    outs, wins = F.window16(imgs, w, return_window=True, device=dev)
    assert len(outs) == len(wins) == len(imgs)
    for i, im in enumerate(imgs):
        want, want_win = W.reference(im, w, return_window=True)
        assert wins[i] == want_win, f"mixed[{i}]"
        _check(outs[i], want, f"mixed[{i}] {wname}")
    again, wins2 = F.window16(imgs, w, return_window=True, device=dev)
    assert wins2 == wins
    for a, b in zip(outs, again):
        assert torch.equal(a, b)
    for i in (0, 3, len(imgs) - 1):
        (alone,), (win,) = F.window16([imgs[i]], w, return_window=True, device=dev)
        assert win == wins[i] and torch.equal(alone, outs[i])
    rev, wins_r = F.window16(imgs[::-1], w, return_window=True, device=dev)
    assert wins_r == wins[::-1]
    for a, b in zip(outs, rev[::-1]):
        assert torch.equal(a, b)


def test_window_passes_returns_device_windows_and_leaves_the_workspace_zero(dev):
    w = W.Window(low=2, high=97)
    planes = mixed_batch() + [image("gauss12_big")]
    descs, src, dst = W.plan(planes, w)
    host = np.zeros(src, np.uint8)
    W.pack(planes, descs, host)
    px = torch.from_numpy(host).to(dev)
    with torch.cuda.device(dev):
        out, wins = F.window_passes(px, descs)
        ws = F._window_workspace(len(planes), dev)
        assert int(ws.view(torch.int32).abs().max()) == 0
        out2, wins2 = F.window_passes(px.view(torch.int16), descs)
    assert out.dtype == torch.uint8 and out.numel() == dst
    assert wins.dtype == torch.int32 and tuple(wins.shape) == (len(planes), 2) and wins.is_cuda
    assert torch.equal(out, out2) and torch.equal(wins, wins2)
    for d, a, win in zip(descs, planes, wins.cpu().tolist()):
        want, want_win = W.reference(a, w, return_window=True)
        assert tuple(win) == want_win
        o = int(d["dst_off"])
        _check(out[o:o + a.size].view(a.shape), want, "window_passes")
    fixed = W.Window("fixed", lo=-0.5, hi=4095.5)
    fdescs, _, _ = W.plan(planes, fixed)
    with torch.cuda.device(dev):
        fout, fwins = F.window_passes(px, fdescs)
    assert fwins is None
    o = int(fdescs[-1]["dst_off"])
    _check(fout[o:].view(planes[-1].shape), W.reference(planes[-1], fixed), "fixed passes")


def test_input_forms(dev):
    from PIL import Image
    img = np.array(image("gauss12_37x53"))
    w = W.Window()
    outs = F.window16([img, img[:, :, None], Image.fromarray(img)], w, device=dev)
    want = W.reference(img, w)
    for o in outs:
        _check(o, want, "input form")


def test_c_entries_reject_bad_tables_before_any_launch(dev):
    from mmdx._lib import call, ptr, stream
    planes = [image("uniform_37x53"), image("uniform_3x5")]
    descs, src, dst = W.plan(planes, W.Window())
    with torch.cuda.device(dev):
        px = torch.zeros(src, dtype=torch.uint8, device=dev)
        dd = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
        out = torch.zeros(dst, dtype=torch.uint8, device=dev)
        lv = torch.zeros((2, 4), dtype=torch.int32, device=dev)
        ws = F._window_workspace(2, dev)

        def levels(d, px_bytes=src, ws_bytes=None):
            call("mmdx_window_levels", ptr(px), px_bytes, d.ctypes.data, ptr(dd), 2, ptr(ws),
                 ws.numel() if ws_bytes is None else ws_bytes, ptr(lv), stream())

        def apply(d, out_bytes=dst, lev=lv):
            call("mmdx_window_apply", ptr(px), src, d.ctypes.data, ptr(dd), 2, ptr(lev),
                 ptr(out), out_bytes, stream())

        for field, value in (("src_off", 8), ("k_hi", 37 * 53), ("k_lo", -1), ("w", 0),
                             ("h", 65536), ("mode", 2), ("invert", 2)):
            bad = descs.copy()
            bad[0][field] = value
            with pytest.raises(RuntimeError):
                levels(bad)
            with pytest.raises(RuntimeError):
                apply(bad)
        with pytest.raises(RuntimeError):
            levels(descs, px_bytes=src - 16)
        with pytest.raises(RuntimeError):
            levels(descs, ws_bytes=2 * 65536 * 4 - 1)
        with pytest.raises(RuntimeError):
            apply(descs, out_bytes=dst - 1)
        with pytest.raises(RuntimeError):      # percentile descriptors need the levels
            apply(descs, lev=None)
        bad = descs.copy()
        bad[1]["dst_off"] = 1                   # overlaps image 0's output
        with pytest.raises(RuntimeError):
            apply(bad)
        fixed, _, _ = W.plan(planes, W.Window("fixed", lo=0, hi=100))
        with pytest.raises(RuntimeError):      # the levels entry takes percentile descriptors
            levels(fixed)
        bad = fixed.copy()
        bad[0]["scale"] = 2.5
        with pytest.raises(RuntimeError):
            apply(bad, lev=None)
        torch.cuda.synchronize()
        assert int(out.max()) == 0 and int(ws.view(torch.int32).abs().max()) == 0


# ----------------------------------------------------------------------------- preprocess
def _batch16():
    """16-bit images large enough for the 224 crop, three sizes (one odd) and pixel classes."""
    from window_cases import gauss12, radiograph, uniform
    return [radiograph((301, 277), 40), gauss12((256, 320), 41), uniform((225, 224), 42)]


def _host_windowed(imgs, w):
    return [W.reference(im, w) for im in imgs]


def test_preprocess_batch_with_window_equals_host_windowing_first(dev):
    imgs = _batch16()
    got = None
    for w in (W.Window(), W.Window(low=0, high=100, invert=True),
              W.Window.from_center_width(1800, 1201), W.Window("fixed", lo=-100.5, hi=70000)):
        got = mmdx.preprocess_batch(imgs, dev, window=w)
        want = mmdx.preprocess_batch(_host_windowed(imgs, w), dev)
        assert got.shape == (3, 3, 224, 224)
        assert torch.equal(got, want), str(w)
    from PIL import Image
    pil = [Image.fromarray(im) for im in imgs]
    assert torch.equal(mmdx.preprocess_batch(pil, dev, window=w), got)
    # window=None: the bits the function gave before, and 16-bit input is rejected as before
    eight = _host_windowed(imgs, W.Window())
    plain = mmdx.preprocess_batch(eight, dev)
    assert torch.equal(mmdx.preprocess_batch(eight, dev, window=None), plain)
    assert torch.equal(mmdx.preprocess_batch(eight, dev, clahe=None, window=None), plain)
    with pytest.raises(TypeError):
        mmdx.preprocess_batch(imgs, dev)
    with pytest.raises(ValueError):
        mmdx.preprocess_batch(pil, dev)
    # mixed depths are out of scope: the TypeError names the index
    with pytest.raises(TypeError, match="image 1"):
        mmdx.preprocess_batch([imgs[0], eight[1], imgs[2]], dev, window=W.Window())
    with pytest.raises(TypeError, match="image 2"):
        mmdx.preprocess_batch([pil[0], imgs[1], Image.fromarray(eight[2], "L")], dev,
                              window=W.Window())


def test_preprocess_batch_with_window_and_clahe(dev):
    imgs = _batch16()
    w, c = W.Window(low=1, high=99), mmdx.Clahe(2.0, (8, 8))
    got = mmdx.preprocess_batch(imgs, dev, clahe=c, window=w)
    host = [c(a) for a in _host_windowed(imgs, w)]
    assert torch.equal(got, mmdx.preprocess_batch(host, dev))
    assert torch.equal(got, mmdx.preprocess_batch(_host_windowed(imgs, w), dev, clahe=c))
    assert not torch.equal(got, mmdx.preprocess_batch(imgs, dev, window=w))
    with pytest.raises(ValueError):     # CLAHE's limits still raise before anything is launched
        mmdx.preprocess_batch([np.zeros((300, 20), np.uint16)] + imgs, dev,
                              clahe=mmdx.Clahe(2.0, (16, 16)), window=w)


def test_loader_on_16_bit_pngs_yields_the_host_windowed_images(dev, tmp_path):
    import pandas as pd
    from PIL import Image
    from mmdx import data as D
    w, c = W.Window(low=0.5, high=99.5), mmdx.Clahe(2.0, (4, 4))
    imgs = _batch16()
    keys = []
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(tmp_path / f"img{i}.png")
        keys.append(f"img{i}.png")
    vecs = [np.eye(13)[i % 13].tolist() for i in range(len(keys))]
    df = pd.DataFrame(dict(image_url=keys, patient_details=[f"p{i}" for i in range(len(keys))],
                           disease_classification_vector=vecs, report=["r"] * len(keys)))
    df = D.enforce_raw_data_columns(df)
    kw = dict(batch_size=2, shuffle=False, device=dev)
    decoded = [D.open_image(str(tmp_path), k) for k in keys]
    assert {im.mode for im in decoded} == {"I;16"}
    assert all(np.array_equal(np.asarray(d), im) for d, im in zip(decoded, imgs))
    loader = D.LocalCXRBatches(df, str(tmp_path), window=w, **kw)
    assert loader.window is w and loader.clahe is None
    got = torch.cat([b[0] for b in loader])
    assert torch.equal(got, mmdx.preprocess_batch(_host_windowed(imgs, w), dev))
    both = torch.cat([b[0] for b in D.LocalCXRBatches(df, str(tmp_path), window=w, clahe=c,
                                                      **kw)])
    assert torch.equal(both, mmdx.preprocess_batch([c(a) for a in _host_windowed(imgs, w)],
                                                   dev))
    with pytest.raises(ValueError):     # without a window 16-bit files are rejected as before
        next(iter(D.LocalCXRBatches(df, str(tmp_path), **kw)))
    with pytest.raises(TypeError):
        D.LocalCXRBatches(df, str(tmp_path), window=w.config(), **kw)


# ----------------------------------------------------------------------------- the bundle
def test_inference_serves_the_bundles_window(dev, tmp_path):
    from PIL import Image
    from mmdx.inference_pipeline import inference, load_model_bundle, save_model_bundle
    torch.manual_seed(0)
    img = mmdx.ImageEncoderCNN("resnet18", 1024, 13).to(dev).eval()
    txt = mmdx.TextEncoderTransformer("bert-base-uncased@2", 512, 13).to(dev).eval()
    fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13).to(dev).eval()
    w = W.Window(low=1, high=99)
    arts = {"class_names": list(mmdx.DISEASES), "thresholds": [0.5] * 13}
    p_w = save_model_bundle(fus, img, txt, str(tmp_path / "w"), timestamped_copy=False,
                            artifacts=dict(arts, window=w.config()))
    p_raw = save_model_bundle(fus, img, txt, str(tmp_path / "raw"), timestamped_copy=False,
                              artifacts=arts)
    b_w = load_model_bundle(p_w, with_report_head=False)
    b_raw = load_model_bundle(p_raw, with_report_head=False)
    assert b_w["window"] == w.config() and b_raw["window"] is None
    img16 = _batch16()[0]
    pil8 = Image.fromarray(W.reference(img16, w))
    r_w = inference(b_w, img16, TEXT)
    r_pil = inference(b_w, Image.fromarray(img16), TEXT)
    r_host = inference(b_raw, pil8, TEXT)
    assert set(r_w) == set(r_host)
    assert r_w["disease_probs"] == r_host["disease_probs"] == r_pil["disease_probs"]
    assert r_w["disease_vector"] == r_host["disease_vector"]
    with pytest.raises(ValueError, match="16-bit"):
        inference(b_w, pil8, TEXT)
    # a bundle dict from before the key behaves as it did
    no_key = {k: v for k, v in b_raw.items() if k != "window"}
    assert inference(no_key, pil8, TEXT)["disease_probs"] == r_host["disease_probs"]
