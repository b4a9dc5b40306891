"""-m gpu: whole-scene prediction -- the two kernels of csrc/scene.hip against the CPU transform and against the kernels they
replace, ScenePredictor end to end against infer.ss_inference / ms_inference on a conditioned ResNet-18, and the command line in a child
process.  Everything compared here is integer or bit-exact except the overlay, whose fp32 blend may land one grey level from float64."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                  # noqa: E402
from emrt_amd.functional import P                          # noqa: E402
from emrt_amd.runtime import F32                           # noqa: E402
from emrt_amd.src.transforms import Normalize              # noqa: E402
from emrt_amd.src.utils import vis                         # noqa: E402
from tests.hip_utils import init, rank_processes           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "emrt_amd/configs/EMRT")
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]          # VAL.MEAN / VAL.STD of every shipped config
STDINV = [float(v) for v in 1.0 / np.asarray(STD, dtype=np.float64)]


def _origins(org):
    arr = (ctypes.c_int * max(2, 2 * len(org)))(*[v for yx in org for v in yx])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _refused(name, message, *args):
    with pytest.raises(_lib.EmrtHipError) as e:
        _lib.lib().call(name, *args)
    assert message in str(e.value) and "launch failed" not in str(e.value), str(e.value)


def _normalised_chw(u8_hwc):
    """transforms.Normalize on the CPU, as the validation pipeline applies it -> fp32 CHW tensor"""
    out = Normalize(MEAN, STD)(np.asarray(u8_hwc, dtype=np.float32))[0]
    return torch.from_numpy(np.ascontiguousarray(np.transpose(out, (2, 0, 1))))


# ---- 1. crop and normalise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch,cw", [(16, 20), (16, 18)])          # cw % 4 == 0: four x per thread; 18: one x per thread
def test_crop_windows_u8_equals_the_cpu_normalize_bit_for_bit(ch, cw):
    c = init(F32)
    L = _lib.lib()
    g = torch.Generator().manual_seed(4001)
    H, W = 37, 45                                            # the width is no multiple of 4: window rows start at any byte
    scene = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    scene[0, 0] = torch.tensor([0, 255, 0], dtype=torch.uint8)          # both ends of the byte range
    org = [(0, 0), (H - ch, W - cw), (5, 3)]                 # the second is flush with the bottom-right corner
    sd = scene.cuda()
    batch = torch.full((len(org), 3, ch, cw), -7.0, device="cuda")
    arr, ptr = _origins(org)
    L.call("emrt_scene_crop_windows_u8", P(sd), P(batch), ptr, len(org), H, W, ch, cw, *MEAN, *STDINV, c.stream)
    want = torch.stack([_normalised_chw(scene.numpy()[y:y + ch, x:x + cw]) for y, x in org])
    assert want.dtype == torch.float32 and torch.equal(batch.cpu(), want)
    # refusals: a window that reaches outside by one pixel (right, bottom), a negative origin, no window, 65 windows, a null pointer
    batch.fill_(-7.0)
    msg = "1..64 windows inside the image"
    for bad in ((0, W - cw + 1), (H - ch + 1, 0), (-1, 0)):
        arr1, ptr1 = _origins([(3, 4), bad])
        _refused("emrt_scene_crop_windows_u8", msg, P(sd), P(batch), ptr1, 2, H, W, ch, cw, *MEAN, *STDINV, c.stream)
    _refused("emrt_scene_crop_windows_u8", msg, P(sd), P(batch), ptr, 0, H, W, ch, cw, *MEAN, *STDINV, c.stream)
    arr65, ptr65 = _origins([(0, 0)] * 65)
    _refused("emrt_scene_crop_windows_u8", msg, P(sd), P(batch), ptr65, 65, H, W, ch, cw, *MEAN, *STDINV, c.stream)
    _refused("emrt_scene_crop_windows_u8", "null pointer", None, P(batch), ptr, 1, H, W, ch, cw, *MEAN, *STDINV, c.stream)
    torch.cuda.synchronize()
    assert float((batch + 7.0).abs().max()) == 0.0, "a refused call must not launch"


# ---- 2. finish against the existing kernels -------------------------------------------------------------------------------------------
ALPHA = float(np.float32(0.3))          # no dyadic fraction: the blend really rounds


def _palette(C, g):
    pal = torch.randint(0, 256, (C, 3), generator=g, dtype=torch.uint8)
    pal[0] = torch.tensor([255, 255, 255], dtype=torch.uint8)
    if C > 1:
        pal[C - 1] = torch.tensor([0, 0, 0], dtype=torch.uint8)
    return pal


def _pal_ptr(pal):
    arr = (ctypes.c_ubyte * pal.numel())(*pal.reshape(-1).tolist())
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _finish(values, count, pal, scene, alpha, offset, areas=None, want=("color", "overlay", "areas")):
    """One emrt_scene_finish launch on device tensors -> (index, color, overlay, areas) on the device.  offset = 1: every output buffer is a
    view one element into its allocation (no output is 4-byte aligned: the one-pixel-per-thread kernel)."""
    c = init(F32)
    N, C, H, W = values.shape

    def buf(*shape):
        raw = torch.full((int(np.prod(shape)) + offset,), 0xAB, dtype=torch.uint8, device="cuda")
        return raw[offset:].view(*shape)

    index = buf(N, H, W)
    color = buf(N, H, W, 3) if "color" in want else None
    overlay = buf(N, H, W, 3) if "overlay" in want else None
    if areas is None and "areas" in want:
        areas = torch.zeros(C, dtype=torch.int64, device="cuda")
    arr, pp = _pal_ptr(pal)
    _lib.lib().call("emrt_scene_finish", P(values), P(count), pp, P(scene), alpha, P(index), P(color), P(overlay), P(areas), N, C, H, W, c.stream)
    return index, color, overlay, areas


def _reference_index(values, count):
    """emrt_window_normalise (when there is a count) + emrt_argmax_nchw: the pair the finish replaces, unchanged, on the same buffers"""
    c = init(F32)
    N, C, H, W = values.shape
    logits = values
    if count is not None:
        assert N == 1
        logits = torch.empty_like(values)
        _lib.lib().call("emrt_window_normalise", P(values), P(count), P(logits), C, H, W, c.stream)
    pred = torch.full((N, 1, H, W), -1, dtype=torch.int32, device="cuda")
    _lib.lib().call("emrt_argmax_nchw", P(logits), P(pred), N, C, H, W, c.stream)
    return pred[:, 0].long()


def _inputs(C, H, W, N, with_count, seed):
    """random sums (and counts from {1..4}) with the planted pixels -> (values, count, {flat pixel of image 0: expected index})"""
    g = torch.Generator().manual_seed(seed)
    values = torch.randn(N, C, H, W, generator=g) * 3
    count = torch.randint(1, 5, (N, H, W), generator=g).float() if with_count else None
    planted = {}
    flat = values[0].view(C, H * W)
    if C >= 2:
        lo, hi = C // 3, C - 1
        flat[:, 1] = -1.0
        flat[lo, 1] = flat[hi, 1] = 50.0                    # the two largest classes are equal: the lower index wins
        planted[1] = lo
        flat[hi, 3] = float("inf")
        planted[3] = hi
    if with_count:
        flat[:, 4] = 0.0
        count.view(-1)[4] = 0.0                              # nobody covered it: 0 / 0 = NaN in every class -> class 0
        planted[4] = 0
    if C >= 4:
        flat[3, H * W - 1] = float("nan")                   # NaN in class 3 only: it counts as the maximum
        planted[H * W - 1] = 3
    return values, count, planted


# the issue's shapes, plus two that take the four-pixels-per-lane kernel over several blocks (the last with a grid-stride step: > 2048 blocks)
FINISH_SHAPES = [(1, 5, 7), (6, 5, 7), (7, 16, 32), (19, 3, 130), (6, 9, 260)]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("N,with_count", [(1, True), (3, False)])
@pytest.mark.parametrize("C,H,W", FINISH_SHAPES)
def test_finish_equals_normalise_argmax_palette_and_bincount(C, H, W, N, with_count, offset):
    values, count, planted = _inputs(C, H, W, N, with_count, 4100 + C + W)
    g = torch.Generator().manual_seed(4200 + C)
    pal = _palette(C, g)
    scene = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    vd, cd, sd = values.cuda(), None if count is None else count.cuda(), scene.cuda()
    ref = _reference_index(vd, cd).cpu()
    index, color, overlay, areas = _finish(vd, cd, pal, sd, ALPHA, offset)
    got = index.cpu().long()
    assert torch.equal(got, ref)
    for pix, cls in planted.items():
        assert int(got[0].view(-1)[pix]) == cls, (pix, cls, int(got[0].view(-1)[pix]))
    want_color = pal[got]
    assert torch.equal(color.cpu(), want_color)
    hist = torch.bincount(got.view(-1), minlength=C)
    assert torch.equal(areas.cpu(), hist)
    # overlay: floor(alpha * color + (1 - alpha) * scene + 0.5); the kernel's fp32 (possibly contracted) blend may cross a .5 boundary
    exact = torch.floor(ALPHA * want_color.double() + (1.0 - ALPHA) * scene.double() + 0.5)
    err = (overlay.cpu().double() - exact).abs().max().item()
    print("overlay C=%d %dx%d N=%d offset=%d: max |kernel - float64| = %g grey levels" % (C, H, W, N, offset, err))
    assert err <= 1.0
    # a second launch: the same bits, and the areas are ADDED to
    index2, color2, overlay2, areas2 = _finish(vd, cd, pal, sd, ALPHA, offset, areas=areas)
    assert torch.equal(index2, index) and torch.equal(color2, color) and torch.equal(overlay2, overlay)
    assert areas2.data_ptr() == areas.data_ptr() and torch.equal(areas.cpu(), 2 * hist)
    # the ends of the blend are exact
    assert torch.equal(_finish(vd, cd, pal, sd, 1.0, offset)[2].cpu(), want_color)
    assert torch.equal(_finish(vd, cd, pal, sd, 0.0, offset)[2].cpu(), scene)
    # outputs nobody asked for are not needed: index alone
    only = _finish(vd, cd, pal, None, 0.0, offset, want=())
    assert only[1] is None and only[2] is None and only[3] is None and torch.equal(only[0], index)


def test_finish_grid_stride_and_one_class_regions():
    """2.36 M pixels: 2304 blocks' worth of quads on a grid capped at 2048, so the stride loop takes a second step; large one-class regions
    (every lane of a wave holds the same classes: the wave adds to the block's histogram once) beside noise."""
    g = torch.Generator().manual_seed(4300)
    N, C, H, W = 2, 3, 1152, 1024
    values = torch.randn(N, C, H, W, generator=g)
    values[0, 1, :600] += 100.0                              # 600 rows of class 1
    values[1, 2, 300:] += 100.0                              # 852 rows of class 2
    pal = _palette(C, g)
    vd = values.cuda()
    ref = _reference_index(vd, None)
    index, color, _, areas = _finish(vd, None, pal, None, 0.0, 0, want=("color", "areas"))
    assert torch.equal(index.long(), ref)
    assert torch.equal(color, pal.cuda()[ref])
    hist = torch.bincount(ref.view(-1), minlength=C)
    assert torch.equal(areas, hist) and int(areas.sum()) == N * H * W and int(hist[1]) > 600 * W


def test_finish_refusals():
    c = init(F32)
    g = torch.Generator().manual_seed(4400)
    N, C, H, W = 1, 6, 4, 8
    values = torch.randn(N, C, H, W, generator=g).cuda()
    scene = torch.zeros(N, H, W, 3, dtype=torch.uint8, device="cuda")
    index = torch.full((N, H, W), 0xAB, dtype=torch.uint8, device="cuda")
    color = torch.full((N, H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    overlay = torch.full((N, H, W, 3), 0xAB, dtype=torch.uint8, device="cuda")
    areas = torch.zeros(C, dtype=torch.int64, device="cuda")
    arr, pp = _pal_ptr(_palette(256, g))
    st = c.stream

    def call(message, values=P(values), pal=pp, scene=P(scene), alpha=0.5, index=P(index), overlay=P(overlay), N=N, C=C, H=H, W=W):
        _refused("emrt_scene_finish", message, values, None, pal, scene, alpha, index, P(color), overlay, P(areas), N, C, H, W, st)

    call("C must be 1..256", C=0)
    call("C must be 1..256", C=257)
    call("null pointer", values=None)
    call("null pointer", index=None)
    call("null pointer", pal=None)
    call("overlay needs scene", scene=None)
    call("alpha must be in [0, 1]", alpha=-0.01)
    call("alpha must be in [0, 1]", alpha=1.01)
    call("alpha must be in [0, 1]", alpha=float("nan"))
    call("N * H * W must be below 2^31", N=2, H=32768, W=32768)
    call("N, H, W must be positive", H=0)
    torch.cuda.synchronize()
    assert int(areas.sum()) == 0 and bool((index == 0xAB).all()) and bool((color == 0xAB).all()) and bool((overlay == 0xAB).all())


# ---- 3. end to end against ss_inference / ms_inference ----------------------------------------------------------------------------------
CROP, STRIDE, NCLS = (64, 64), (32, 32), 6


@pytest.fixture(scope="module")
def resnet18():
    """ResNet-18 EMRT, 6 classes, fp32, residual branches conditioned and BatchNorm statistics calibrated as tests/test_gpu_model.py does"""
    from tests.test_gpu_model import build_pair
    g = torch.Generator().manual_seed(4500)
    x = torch.randn(2, 3, 64, 64, generator=g)
    _, model = build_pair("resnet18", x, condition=0.1)
    model.eval()
    return model


@pytest.fixture(scope="module")
def scene_100x170():
    g = torch.Generator().manual_seed(4501)
    return torch.randint(0, 256, (100, 170, 3), generator=g, dtype=torch.uint8)


def _predictor(model, **kw):
    from emrt_amd.src.api.scene import ScenePredictor
    return ScenePredictor(model, NCLS, CROP, STRIDE, vis.get_palette("Potsdam"), MEAN, STD, **kw)


def test_scene_predictor_equals_ss_inference(resnet18, scene_100x170):
    from emrt_amd.src.api import infer
    scene = scene_100x170
    assert max(w[0] for w in infer.window_grid(100, 170, CROP, STRIDE)) == 36          # the edge windows are shifted back inside: counts reach 4
    img = _normalised_chw(scene.numpy()).cuda()
    want = infer.ss_inference(resnet18, [img], [(100, 170)], True, None, STRIDE, CROP, NCLS)[0]
    res = _predictor(resnet18)(scene.cuda())                 # the default max_batch: chunked as ss_inference chunks, the same logits
    index = res.index.long().cpu()
    assert torch.equal(index, want[0, 0].long().cpu())
    assert res.overlay is None and int(res.areas.sum()) == 17000
    assert torch.equal(res.areas.cpu(), torch.bincount(index.view(-1), minlength=NCLS))
    assert len(torch.unique(index)) > 1, "a one-class map would compare nothing"
    pal = torch.from_numpy(vis.get_palette("Potsdam"))
    assert torch.equal(res.color.cpu(), pal[index])
    over = _predictor(resnet18, overlay=0.5)(scene.cuda())
    assert torch.equal(over.index, res.index) and torch.equal(over.color, res.color) and torch.equal(over.areas, res.areas)
    exact = torch.floor(0.5 * pal[index].double() + 0.5 * scene.double() + 0.5)          # (0.5 is dyadic: the fp32 blend is exact)
    assert torch.equal(over.overlay.cpu().double(), exact)


def test_predict_tiles_equals_the_model_on_each_tile(resnet18):
    g = torch.Generator().manual_seed(4502)
    tiles = torch.randint(0, 256, (3, 64, 64, 3), generator=g, dtype=torch.uint8)
    norm = torch.stack([_normalised_chw(t.numpy()) for t in tiles]).cuda()
    single = torch.stack([resnet18(norm[j:j + 1])[0][0].argmax(0) for j in range(3)]).cpu()
    res1 = _predictor(resnet18, max_batch=1).predict_tiles(tiles.cuda())          # three model calls of one tile: the same launches
    assert torch.equal(res1.index.long().cpu(), single)
    together = resnet18(norm)[0].argmax(1).cpu()
    res = _predictor(resnet18).predict_tiles(tiles.cuda())                        # one model call of three tiles
    assert torch.equal(res.index.long().cpu(), together)
    assert res.index.shape == (3, 64, 64) and res.color.shape == (3, 64, 64, 3) and int(res.areas.sum()) == 3 * 64 * 64
    res2 = _predictor(resnet18, max_batch=2).predict_tiles(tiles.cuda())          # chunks of 2 + 1 written into one result, areas summed
    assert int(res2.areas.sum()) == 3 * 64 * 64
    assert torch.equal(res2.areas.cpu(), torch.bincount(res2.index.long().view(-1), minlength=NCLS).cpu())
    assert torch.equal(res2.index[2], res1.index[2])


def test_scene_predictor_multi_scale_equals_ms_inference(resnet18, scene_100x170):
    from emrt_amd.src.api import infer
    scene = scene_100x170
    img = _normalised_chw(scene.numpy()).cuda()
    want = infer.ms_inference(resnet18, [img], (100, 170), True, None, STRIDE, CROP, NCLS, scales=[0.75, 1.0])
    res = _predictor(resnet18, scales=(0.75, 1.0))(scene.cuda())
    assert torch.equal(res.index.long().cpu(), want[0, 0].long().cpu())
    assert int(res.areas.sum()) == 17000


# ---- 4. the command line ------------------------------------------------------------------------------------------------------------
def test_predict_cli_writes_colour_overlay_and_index_pngs(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_fake_potsdam
    finally:
        sys.path.pop(0)
    import argparse
    from emrt_amd.config import get_config, update_config
    from emrt_amd.src.models import get_model
    from emrt_amd.src.utils.checkpoint import save_pdparams
    root = make_fake_potsdam.make(str(tmp_path / "potsdam"), n_train=1, n_val=3, size=64)
    cfg = str(tmp_path / "tiny.yaml")
    with open(cfg, "w") as f:
        f.write('BASE: ["%s"]\n' % os.path.relpath(os.path.join(CFG_DIR, "EMRT_256x256_160k_potsdam.yaml"), str(tmp_path)))
        f.write('DATA: {CROP_SIZE: "(64, 64)", DATA_PATH: "%s"}\n' % root)
        f.write('MODEL: {ENCODER: {TYPE: "resnet18"}}\n')
        f.write("VAL: {IMAGE_BASE_SIZE: 64, CROP_SIZE: [64, 64], STRIDE_SIZE: [64, 64]}\n")
        f.write('SAVE_DIR: "%s"\n' % str(tmp_path / "run"))
    torch.manual_seed(0)
    ckpt = str(tmp_path / "model.pdparams")
    save_pdparams(get_model(update_config(get_config(), argparse.Namespace(cfg=cfg))).state_dict(), ckpt)
    with rank_processes(1):
        r = subprocess.run([sys.executable, "-m", "emrt_amd.predict", "--config", cfg, "--model_path", ckpt, "--overlay", "0.5", "--save_index"],
                           cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = str(tmp_path / "run" / "predict")                 # the default: <SAVE_DIR>/predict
    assert sorted(os.listdir(out)) == sorted("%d%s.png" % (i, s) for i in range(3) for s in ("", "_overlay", "_index"))
    assert r.stdout.count("class share:") == 3 and "[PREDICT] Images: 3  files written: 9" in r.stdout
    pal = vis.get_palette("Potsdam")
    code = {tuple(int(v) for v in c): k for k, c in enumerate(pal)}
    for i in range(3):
        with Image.open(os.path.join(root, "test", "%d.tif" % i)) as im:
            size = im.size
        with Image.open(os.path.join(out, "%d.png" % i)) as im:
            assert im.mode == "RGB" and im.size == size
            color = np.asarray(im)
        with Image.open(os.path.join(out, "%d_overlay.png" % i)) as im:
            assert im.mode == "RGB" and im.size == size
        with Image.open(os.path.join(out, "%d_index.png" % i)) as im:
            assert im.mode == "P" and im.size == size
            index = np.asarray(im)
            assert im.getpalette()[:18] == pal.reshape(-1).tolist()
        colours = {tuple(int(v) for v in c) for c in color.reshape(-1, 3)}
        assert colours <= set(code), colours - set(code)     # every colour is a palette entry
        back = np.vectorize(lambda r_, g_, b_: code[(r_, g_, b_)])(color[..., 0], color[..., 1], color[..., 2])
        assert np.array_equal(back, index)
