"""GPU tests of sfgs.depthvis (csrc/depthvis.hip): the depth colorisation of render_video.py:129-170 and the frame quantiser
of render_video.py:264. The bar is EQUALITY: every pixel of both output kinds equals, bit for bit, the reference's own run
(tests/golden/make_golden_depthvis.py) and the float32 restatement in tests/depthvis_np.py (which tests/test_depthvis_host.py
holds to the golden and, where the reference is present, to the live reference). Nothing here reads the reference tree or
matplotlib."""
import os
import types

import numpy as np
import pytest
import torch

import depthvis_np as dnp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_depthvis.npz")
_G = np.load(GOLDEN)
TAGS = sorted(k[:-len("_depth")] for k in _G.files if k.endswith("_depth"))
SIZES = [(1080, 1920), (1024, 1024), (2160, 3840), (1079, 1917)]
FULL_KINDS = dnp.KINDS + ("few", "special")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_both(depth, mask=None, normalize=True, **kw):
    """-> (float32 [3,H,W], uint8 [H,W,3]) as numpy, from two calls of the operator"""
    from sfgs import depthvis
    d = torch.from_numpy(np.ascontiguousarray(depth)).to(DEV)
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    f = depthvis.colorize_depth(d[None], None if m is None else m[None], normalize=normalize, out="float_chw", **kw)
    u = depthvis.colorize_depth(d, m, normalize=normalize, out="uint8_hwc", **kw)
    assert f.dtype == torch.float32 and tuple(f.shape) == (3,) + depth.shape and f.device == d.device
    assert u.dtype == torch.uint8 and tuple(u.shape) == depth.shape + (3,) and u.device == d.device
    return f.cpu().numpy(), u.cpu().numpy()


def assert_equals_restatement(depth, mask, normalize, lut, what):
    want8, _, _ = dnp.colorize(depth, lut, mask, normalize)
    f, u = run_both(depth, mask, normalize)
    bad = np.argwhere((u != want8).any(axis=2))
    assert bad.size == 0, f"{what}: {len(bad)} uint8 pixels differ, first at {bad[0]}: {u[tuple(bad[0])]} != {want8[tuple(bad[0])]}"
    assert np.array_equal(bits(f), bits(dnp.to_float_chw(want8))), f"{what}: float_chw differs"


@pytest.mark.parametrize("tag", TAGS)
def test_golden_case_bit_for_bit_in_both_output_kinds(tag):
    depth = _G[f"{tag}_depth"]
    mask = _G[f"{tag}_mask"] if f"{tag}_mask" in _G.files else None
    want = _G[f"{tag}_result"]
    f, u = run_both(depth, mask, bool(_G[f"{tag}_normalize"]))
    assert np.array_equal(bits(f), bits(want)), tag
    # the uint8 frame: the same table entries (the golden's floats are k / 255 exactly: recover k)
    want8 = np.rint(want.transpose(1, 2, 0) * 255.0).astype(np.uint8)
    assert np.array_equal(bits((want8.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)), bits(want))
    np.testing.assert_array_equal(u, want8, err_msg=tag)


def test_built_in_table_on_the_device_is_the_golden_table():
    from sfgs import depthvis
    lut = depthvis._device_lut("Spectral", torch.device(DEV))
    assert lut is depthvis._device_lut("Spectral", torch.device(DEV))      # cached per device
    np.testing.assert_array_equal(lut.cpu().numpy(), _G["spectral_lut"])


@pytest.mark.parametrize("kind", FULL_KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_full_size_frames_equal_the_restatement_bit_for_bit(H, W, kind):
    lut = _G["spectral_lut"]
    seed = 7000 + 13 * H + W + 101 * FULL_KINDS.index(kind)
    depth = dnp.make_depth(kind, H, W, seed)
    if kind == "few":
        assert 0 < (depth > 0).sum() < 64
    for mask in (None, dnp.make_mask(H, W, seed)):
        assert_equals_restatement(depth, mask, True, lut, f"{kind} {H}x{W} mask={mask is not None}")


@pytest.mark.parametrize("H,W", [(1080, 1920), (1079, 1917), (3, 1), (1, 67), (64, 64)])
def test_normalize_off_and_a_caller_table(H, W):
    from sfgs import depthvis
    rng = np.random.default_rng(H * W)
    depth = (dnp.make_depth("special" if H * W > 100 else "uniform", H, W, 31) / np.float32(50)).astype(np.float32)   # 1 - disp spread over [0, 1]
    mask = dnp.make_mask(H, W, 31).astype(np.uint8) * np.uint8(7)             # a uint8 mask: non-zero = use the pixel
    assert_equals_restatement(depth, None, False, _G["spectral_lut"], "raw")
    assert_equals_restatement(depth, mask, False, _G["spectral_lut"], "raw masked")
    table = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    want8, _, _ = dnp.colorize(depth, table, mask, True)
    d, m = torch.from_numpy(depth).to(DEV), torch.from_numpy(mask).to(DEV)
    got = depthvis.colorize_depth(d, m, lut=torch.from_numpy(table).to(DEV), out="uint8_hwc")
    np.testing.assert_array_equal(got.cpu().numpy(), want8)


def test_unaligned_and_non_contiguous_inputs():
    """A depth map that starts 4 bytes into an allocation (the 16-byte vector path does not apply although H * W % 4 == 0), a
    mask that starts 1 byte in, and a strided view (made contiguous by the operator)."""
    from sfgs import depthvis
    H, W = 96, 128
    depth = dnp.make_depth("smooth", H, W, 77)
    mask = dnp.make_mask(H, W, 77)
    want8, _, _ = dnp.colorize(depth, _G["spectral_lut"], mask)
    buf = torch.zeros(H * W + 1, dtype=torch.float32, device=DEV)
    buf[1:] = torch.from_numpy(depth).to(DEV).view(-1)
    mbuf = torch.zeros(H * W + 1, dtype=torch.bool, device=DEV)
    mbuf[1:] = torch.from_numpy(mask).to(DEV).view(-1)
    d, m = buf[1:].view(H, W), mbuf[1:].view(H, W)
    assert d.data_ptr() % 16 == 4 and m.data_ptr() % 4 == 1 and d.is_contiguous()
    for out in ("uint8_hwc", "float_chw"):
        got = depthvis.colorize_depth(d, m, out=out).cpu().numpy()
        want = want8 if out == "uint8_hwc" else dnp.to_float_chw(want8)
        np.testing.assert_array_equal(got, want, err_msg=out)
    wide = torch.zeros(H, 2 * W, dtype=torch.float32, device=DEV)
    wide[:, ::2] = torch.from_numpy(depth).to(DEV)
    got = depthvis.colorize_depth(wide[:, ::2], torch.from_numpy(mask).to(DEV), out="uint8_hwc")
    np.testing.assert_array_equal(got.cpu().numpy(), want8)


def test_two_runs_give_identical_bytes():
    from sfgs import depthvis
    H, W = 1080, 1920
    d = torch.from_numpy(dnp.make_depth("smooth", H, W, 5)).to(DEV)
    m = torch.from_numpy(dnp.make_mask(H, W, 5)).to(DEV)
    for out in ("float_chw", "uint8_hwc"):
        runs = [depthvis.colorize_depth(d, m, out=out) for _ in range(3)]
        torch.cuda.synchronize()
        for r in runs[1:]:
            assert torch.equal(r.view(torch.uint8).view(-1), runs[0].view(torch.uint8).view(-1)), out


def test_operator_runs_on_a_non_default_stream():
    from sfgs import depthvis
    H, W = 540, 960
    depth = dnp.make_depth("uniform", H, W, 9)
    want8, _, _ = dnp.colorize(depth, _G["spectral_lut"])
    d = torch.from_numpy(depth).to(DEV)
    img = torch.rand(3, H, W, device=DEV)
    depthvis.colorize_depth(d)                              # table upload and library load on the default stream
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side and side.cuda_stream != 0
        got = depthvis.colorize_depth(d, out="uint8_hwc")
        q = depthvis.quantize_frame(img)
    side.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want8)
    np.testing.assert_array_equal(q.cpu().numpy(), dnp.quantize_frame(img.cpu().numpy()))


def test_install_on_a_stand_in_module_gives_the_direct_call():
    from sfgs import depthvis

    def colorize_depth_torch(depth_tensor, mask=None, normalize=True, cmap='Spectral'):
        raise AssertionError("the original was called")
    mod = types.ModuleType("render_video_stand_in")
    mod.colorize_depth_torch = colorize_depth_torch
    mod.render_frame = lambda depth, **kw: mod.colorize_depth_torch(depth, **kw)   # looks the name up when called
    H, W = 135, 240
    d = torch.from_numpy(dnp.make_depth("smooth", H, W, 3)).to(DEV)[None]
    m = torch.from_numpy(dnp.make_mask(H, W, 3)).to(DEV)[None]
    depthvis.install(mod)
    try:
        for kw in ({}, {"mask": m}, {"normalize": False}, {"mask": m, "normalize": False, "cmap": "Spectral"}):
            got = mod.render_frame(d, **kw)
            direct = depthvis.colorize_depth(d, kw.get("mask"), normalize=kw.get("normalize", True))
            assert got.dtype == torch.float32 and tuple(got.shape) == (3, H, W) and got.device == d.device
            assert torch.equal(got.view(torch.int32), direct.view(torch.int32)), kw
    finally:
        depthvis.uninstall(mod)
    assert mod.colorize_depth_torch is colorize_depth_torch


def rendered_like_frame(H, W, seed):
    """[3,H,W] float32 with values below 0, above 1, NaN, +-inf, and every k / 255 with its two float32 neighbours"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(-0.1, 1.1, (3, H, W)).astype(np.float32)
    flat = img.reshape(-1)
    k = (np.arange(256, dtype=np.float32) / np.float32(255))
    exact = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                            (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)]).astype(np.float32)
    assert flat.size > exact.size + 8
    flat[:exact.size] = exact
    flat[exact.size:exact.size + 8] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 300.0, -300.0]
    return img


@pytest.mark.parametrize("H,W", [(1080, 1920), (37, 53), (1079, 1917)])
def test_quantize_frame_equals_the_numpy_formula(H, W):
    from sfgs import depthvis
    img = rendered_like_frame(H, W, H + W)
    got = depthvis.quantize_frame(torch.from_numpy(img).to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W, 3)
    want = dnp.quantize_frame(img)
    finite = ~np.isnan(img.transpose(1, 2, 0))
    with np.errstate(invalid="ignore"):
        spelled = (img.transpose(1, 2, 0) * 255 + 0.5).clip(0, 255)              # render_video.py:264 before the cast
    np.testing.assert_array_equal(want[finite], spelled[finite].astype(np.uint8))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert got.cpu().numpy()[np.isnan(img.transpose(1, 2, 0))].max() == 0        # NaN -> 0, as the docstring says


def test_frame_downloader_round_trip_of_the_uint8_frame():
    from sfgs import depthvis
    from sfgs.video import FrameDownloader
    H, W = 270, 480
    frames, wants = [], []
    for i in range(4):
        depth = dnp.make_depth("smooth", H, W, 40 + i)
        wants.append(dnp.colorize(depth, _G["spectral_lut"])[0])
        frames.append(torch.from_numpy(depth).to(DEV))
    dl = FrameDownloader(depth=2, device=DEV)
    got = []
    for d in frames:
        got.extend(a.copy() for a in dl.submit(depthvis.colorize_depth(d, out="uint8_hwc")))
    got.extend(a.copy() for a in dl.drain())
    assert len(got) == 4
    for a, w in zip(got, wants):
        assert a.dtype == np.uint8 and a.shape == (H, W, 3)
        np.testing.assert_array_equal(a, w)
