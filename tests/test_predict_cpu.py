"""CPU: the host side of `python -m emrt_amd.predict` -- palettes, the refusals of ScenePredictor, the launches a scene and a stack of tiles
issue (on the recording stand-in tests/fake_abi.py: nothing is computed), the test-split listing, the PNG writers and the argument parser."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ISPRS = [(255, 255, 255), (0, 0, 255), (0, 255, 255), (0, 255, 0), (255, 255, 0), (255, 0, 0)]
LOVEDA = [(255, 255, 255), (255, 0, 0), (255, 255, 0), (0, 0, 255), (159, 129, 183), (0, 255, 0), (255, 195, 128)]
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


# ---- palettes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,want", [("Potsdam", ISPRS), ("Vaihingen", ISPRS), ("LoveDA", LOVEDA)])
def test_palette_values(name, want):
    from emrt_amd.src.utils import vis
    pal = vis.get_palette(name)
    assert isinstance(pal, np.ndarray) and pal.dtype == np.uint8 and pal.shape == (len(want), 3)
    assert pal.tolist() == [list(c) for c in want]


def test_palette_of_an_unknown_dataset_is_refused():
    from emrt_amd.src.utils import vis
    with pytest.raises(ValueError, match="PascalContext"):
        vis.get_palette("PascalContext")


# ---- ScenePredictor on the recording ABI ------------------------------------------------------------------------------------------
class _Model:
    """stands where the network stands: fp32 [n, ncls, h, w] logits for an fp32 [n, 3, h, w] batch, and a count of the calls"""

    def __init__(self, ncls):
        self.ncls, self.batches = ncls, []

    def __call__(self, x):
        self.batches.append(tuple(x.shape))
        return [torch.zeros(x.shape[0], self.ncls, x.shape[2], x.shape[3])]


@pytest.fixture
def fake():
    from tests import fake_abi
    lib = fake_abi.install()
    yield lib
    fake_abi.uninstall()


def _predictor(ncls=6, crop=(64, 64), stride=(32, 32), **kw):
    from emrt_amd.src.api.scene import ScenePredictor
    from emrt_amd.src.utils import vis
    model = _Model(ncls)
    return model, ScenePredictor(model, ncls, crop, stride, vis.get_palette("Potsdam")[:ncls], MEAN, STD, **kw)


def test_stride_larger_than_the_crop_is_refused():
    for stride in ((65, 32), (32, 65)):
        with pytest.raises(ValueError, match="uncovered stripes"):
            _predictor(stride=stride)
    _predictor(stride=(64, 64))


def test_palette_length_must_be_num_classes():
    from emrt_amd.src.api.scene import ScenePredictor
    from emrt_amd.src.utils import vis
    with pytest.raises(ValueError, match=r"palette must be uint8 \[6, 3\]"):
        ScenePredictor(_Model(6), 6, (64, 64), (32, 32), vis.get_palette("LoveDA"), MEAN, STD)
    with pytest.raises(ValueError, match="palette must be uint8"):
        ScenePredictor(_Model(6), 6, (64, 64), (32, 32), vis.get_palette("Potsdam").astype(np.int64), MEAN, STD)


def test_scene_smaller_than_the_crop_is_refused_with_both_sizes(fake):
    _, p = _predictor(crop=(64, 48))                       # (w, h): windows of 48 rows x 64 columns
    for shape in ((47, 200, 3), (200, 63, 3)):
        with pytest.raises(ValueError) as e:
            p(torch.zeros(shape, dtype=torch.uint8))
        assert "%dx%d" % shape[:2] in str(e.value) and "48x64" in str(e.value), str(e.value)
    assert fake.calls == []
    with pytest.raises(ValueError, match="torch.uint8"):
        p(torch.zeros(100, 100, 3))


def _origins_of(args, pos, n):
    arr = ctypes.cast(args[pos], ctypes.POINTER(ctypes.c_int))
    return [(arr[2 * j], arr[2 * j + 1]) for j in range(n)]


def test_single_scale_scene_issues_crop_accumulate_per_chunk_and_one_finish(fake):
    from emrt_amd.src.api import infer
    model, p = _predictor(max_batch=4, overlay=0.5)
    scene = torch.zeros(100, 170, 3, dtype=torch.uint8)
    res = p(scene)
    wins = infer.window_grid(100, 170, (64, 64), (32, 32))
    assert len(wins) == 15                                  # 3 rows x 5 columns, the last of each shifted back inside
    chunks = [wins[i:i + 4] for i in range(0, len(wins), 4)]
    names = [n for n, _ in fake.calls if n != "emrt_memset"]
    assert names == ["emrt_scene_crop_windows_u8", "emrt_window_accumulate"] * len(chunks) + ["emrt_scene_finish"]
    launches = [(n, a) for n, a in fake.calls if n != "emrt_memset"]
    for k, chunk in enumerate(chunks):
        (_, crop), (_, acc) = launches[2 * k], launches[2 * k + 1]
        want = [(a, b) for (a, b, _, _) in chunk]
        assert crop[3:8] == (len(chunk), 100, 170, 64, 64) and _origins_of(crop, 2, len(chunk)) == want
        assert list(crop[8:14]) == MEAN + [1.0 / s for s in STD]
        assert acc[4:10] == (len(chunk), 6, 100, 170, 64, 64) and _origins_of(acc, 3, len(chunk)) == want
    assert model.batches == [(len(chunk), 3, 64, 64) for chunk in chunks]
    fin = launches[-1][1]
    assert fin[1] is not None and fin[1].value                              # a count
    assert fin[3].value == scene.data_ptr() and fin[4] == 0.5               # the overlay blends the scene itself
    assert fin[9:13] == (1, 6, 100, 170)
    assert res.index.shape == (100, 170) and res.index.dtype == torch.uint8
    assert res.color.shape == (100, 170, 3) and res.overlay.shape == (100, 170, 3) and res.color.dtype == torch.uint8
    assert res.areas.shape == (6,) and res.areas.dtype == torch.int64
    assert (fin[5].value, fin[6].value, fin[7].value, fin[8].value) == (res.index.data_ptr(), res.color.data_ptr(), res.overlay.data_ptr(), res.areas.data_ptr())


def test_without_overlay_neither_scene_nor_overlay_reaches_the_kernel(fake):
    _, p = _predictor()
    res = p(torch.zeros(64, 64, 3, dtype=torch.uint8))
    fin = [a for n, a in fake.calls if n == "emrt_scene_finish"]
    assert len(fin) == 1 and fin[0][3] is None and fin[0][7] is None and res.overlay is None


def test_predict_tiles_chunks_the_stack_and_concatenates_in_tile_order(fake):
    model, p = _predictor(max_batch=2)
    tiles = torch.zeros(5, 64, 64, 3, dtype=torch.uint8)
    res = p.predict_tiles(tiles)
    assert model.batches == [(2, 3, 64, 64), (2, 3, 64, 64), (1, 3, 64, 64)]
    crops = [a for n, a in fake.calls if n == "emrt_scene_crop_windows_u8"]
    fins = [a for n, a in fake.calls if n == "emrt_scene_finish"]
    assert "emrt_window_accumulate" not in [n for n, _ in fake.calls]
    assert [a[3] for a in crops] == [2, 2, 1] and all(a[4:8] == (5 * 64, 64, 64, 64) for a in crops)       # one tall scene [n * h][w][3]
    assert [_origins_of(a, 2, a[3]) for a in crops] == [[(0, 0), (64, 0)], [(128, 0), (192, 0)], [(256, 0)]]
    assert [a[9] for a in fins] == [2, 2, 1] and all(a[1] is None for a in fins) and all(a[10:13] == (6, 64, 64) for a in fins)
    assert res.index.shape == (5, 64, 64) and res.color.shape == (5, 64, 64, 3) and res.overlay is None
    for k, j0 in enumerate((0, 2, 4)):                      # every launch writes its own tiles of the one result
        assert fins[k][5].value == res.index[j0].data_ptr() and fins[k][6].value == res.color[j0].data_ptr()
        assert fins[k][8].value == res.areas.data_ptr()     # ... and adds to the same areas
    with pytest.raises(ValueError, match="crop-sized tiles"):
        p.predict_tiles(torch.zeros(2, 64, 32, 3, dtype=torch.uint8))


def test_multi_scale_finishes_the_softmax_sums_without_a_count(fake):
    model, p = _predictor(scales=(0.75, 1.0))
    p(torch.zeros(100, 170, 3, dtype=torch.uint8))
    names = [n for n, _ in fake.calls]
    first = [a for n, a in fake.calls if n == "emrt_scene_crop_windows_u8"]
    assert len(first) == 1 and first[0][3:8] == (1, 100, 170, 100, 170)          # the whole scene as one window
    assert names.count("emrt_softmax_nchw_acc") == 4 and names[-1] == "emrt_scene_finish" and "emrt_argmax_nchw" not in names
    fin = fake.calls[-1][1]
    assert fin[1] is None and fin[9:13] == (1, 6, 100, 170)


# ---- the library's own argument checks (host code: they return before anything touches a device) -----------------------------------
def test_scene_entry_points_refuse_bad_arguments_before_any_launch():
    from emrt_amd import _lib, build_ext
    build_ext.build(verbose=False)
    _lib._LIB = None
    L = _lib.lib()
    p = ctypes.c_void_p(0x10000)          # "a device pointer": aligned, never read
    pal = (ctypes.c_ubyte * 18)(*range(18))
    pp = ctypes.cast(pal, ctypes.c_void_p)

    def finish(match, values=p, pal=pp, scene=p, alpha=0.5, index=p, overlay=p, N=1, C=6, H=4, W=8):
        with pytest.raises(_lib.EmrtHipError, match=match):
            L.call("emrt_scene_finish", values, None, pal, scene, alpha, index, p, overlay, p, N, C, H, W, None)

    finish("C must be 1..256", C=0)
    finish("C must be 1..256", C=257)
    finish("null pointer", values=None)
    finish("null pointer", index=None)
    finish("null pointer", pal=None)
    finish("overlay needs scene", scene=None)
    finish(r"alpha must be in \[0, 1\]", alpha=1.5)
    finish(r"N \* H \* W must be below 2\^31", N=2, H=32768, W=32768)
    org = (ctypes.c_int * 4)(0, 0, 3, 2)
    op = ctypes.cast(org, ctypes.c_void_p)
    norm = MEAN + [1.0 / s for s in STD]
    for n, H, W in ((0, 8, 8), (65, 8, 8), (2, 6, 8), (2, 8, 5)):          # no window, too many, the second one leaves the scene (bottom, right)
        with pytest.raises(_lib.EmrtHipError, match="1..64 windows inside the image"):
            L.call("emrt_scene_crop_windows_u8", p, p, op, n, H, W, 4, 4, *norm, None)
    with pytest.raises(_lib.EmrtHipError, match="null pointer"):
        L.call("emrt_scene_crop_windows_u8", p, None, op, 1, 8, 8, 4, 4, *norm, None)
    _lib._LIB = None


# ---- the test split ---------------------------------------------------------------------------------------------------------------
def test_test_images_lists_the_test_split_in_dataset_order(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_fake_potsdam
    finally:
        sys.path.pop(0)
    from emrt_amd.config import get_config
    from emrt_amd.src import datasets
    root = make_fake_potsdam.make(str(tmp_path / "potsdam"), n_train=2, n_val=11, size=8)
    cfg = get_config()
    cfg.DATA.DATASET, cfg.DATA.DATA_PATH = "Potsdam", root
    got = datasets.test_images(cfg)
    assert got == [os.path.join(root, "test", "%d.tif" % i) for i in range(11)]          # numeric order: 10 after 9, as Dataset lists them
    cfg.DATA.DATASET = "PascalContext"
    with pytest.raises(NotImplementedError):
        datasets.test_images(cfg)


# ---- PNG writers ------------------------------------------------------------------------------------------------------------------
def test_png_writers_round_trip(tmp_path):
    from emrt_amd.src.utils import vis
    rng = np.random.RandomState(0)
    pal = vis.get_palette("LoveDA")
    index = rng.randint(0, 7, (13, 21)).astype(np.uint8)
    color = pal[index]
    vis.save_color_png(str(tmp_path / "c.png"), color)
    vis.save_index_png(str(tmp_path / "i.png"), index, pal)
    with Image.open(str(tmp_path / "c.png")) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), color)
    with Image.open(str(tmp_path / "i.png")) as im:
        assert im.mode == "P" and np.array_equal(np.asarray(im), index)
        assert im.getpalette()[:21] == pal.reshape(-1).tolist()
        assert np.array_equal(np.asarray(im.convert("RGB")), color)
    with pytest.raises(ValueError):
        vis.save_color_png(str(tmp_path / "x.png"), index)
    with pytest.raises(ValueError):
        vis.save_index_png(str(tmp_path / "x.png"), color, pal)


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_parse_args_defaults_and_several_inputs():
    from emrt_amd import predict
    a = predict.parse_args([])
    assert a.cfg.endswith("configs/EMRT/EMRT_256x256_160k_potsdam.yaml") and a.model_path is None and a.multi_scales is False
    assert a.input is None and a.save_dir is None and a.dtype == "fp32" and a.max_batch == 32 and a.overlay is None and a.save_index is False
    a = predict.parse_args(["--input", "a.tif", "tiles", "b.png", "--overlay", "0.25", "--save_index", "--dtype", "bf16", "--max_batch", "8"])
    assert a.input == ["a.tif", "tiles", "b.png"] and a.overlay == 0.25 and a.save_index and a.dtype == "bf16" and a.max_batch == 8


def test_input_files_expands_directories_sorted_and_not_recursively(tmp_path):
    from emrt_amd import predict
    d = tmp_path / "d"
    (d / "sub").mkdir(parents=True)
    for n in ("b.tif", "a.tif", "sub/c.tif"):
        (d / n).write_bytes(b"")
    one = tmp_path / "z.png"
    one.write_bytes(b"")
    assert predict.input_files([str(one), str(d)]) == [str(one), str(d / "a.tif"), str(d / "b.tif")]
    with pytest.raises(ValueError, match="neither a file nor a directory"):
        predict.input_files([str(tmp_path / "missing")])
