"""CPU: multi-scale test-time augmentation of whole-scene inference -- the numpy restatement's own consistency
(tests/ms_tta_reference.py), the sixth library's header, build, loader and host-side refusals, the launches ScenePredictor / SceneEvaluator issue
with tta_scales (on recording stand-ins for the first and the sixth library: nothing is computed), the two command lines' flags, and the share of
pixels the GPU cases leave undecided, judged from the reference alone.  The kernels themselves are held to the restatement in
tests/test_gpu_ms_tta.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import fake_abi
from tests import ms_tta_reference as M
from tests import tta_reference as R
from tests.test_scene_sampler_cpu import write_scene_tree

MEAN, STD = M.MEAN, M.STD
VAL_SUB = ("val_images", "val_labels")
ENTRY = ("emrt_mst_crop_windows_u8", "emrt_mst_window_accumulate")


# ---- the reference itself ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src", [8, 10, 20, 32, 21])
def test_reference_resampling_is_interpolate_bilinear(n_src):
    rng = np.random.RandomState(6000 + n_src)
    a = rng.standard_normal((2, 3, n_src, n_src))
    want = torch.nn.functional.interpolate(torch.from_numpy(a), size=(16, 16), mode="bilinear", align_corners=False).numpy()
    assert np.abs(M.resample(a, 16, 16) - want).max() <= 1e-12
    b = rng.standard_normal((1, 2, n_src, 13))                # a rectangle: the axes are resampled independently
    want = torch.nn.functional.interpolate(torch.from_numpy(b), size=(16, 29), mode="bilinear", align_corners=False).numpy()
    assert np.abs(M.resample(b, 16, 29) - want).max() <= 1e-12
    i0, i1, w = M.taps(16, n_src)
    assert i0.min() >= 0 and i1.max() <= n_src - 1 and np.all((i1 == i0 + 1) | (i1 == n_src - 1)) and np.all((0 <= w) & (w < 1))
    assert w[0] == 0 or n_src > 16                                      # an upsampling clamps its first tap


def test_reference_at_scale_one_is_the_tta_reference_exactly():
    rng = np.random.RandomState(6010)
    i0, i1, w = M.taps(16, 16)
    assert np.array_equal(i0, np.arange(16)) and not w.any()
    scene = rng.randint(0, 256, (37, 41, 3)).astype(np.uint8)
    org, codes = [(0, 0), (21, 25), (5, 3)], R.MODES["d4"]
    assert np.array_equal(M.crop_variants_ms(scene, org, codes, 16, 16, 16, 16), R.crop_variants(scene, org, codes, 16, 16, MEAN, STD))
    logits = rng.standard_normal((len(org) * 8, 5, 16, 16)) * 3
    f, c, b = M.accumulate_ms(logits, org, codes, 37, 41, 16, 16)
    f1, c1 = R.accumulate(logits, org, codes, 37, 41)
    assert np.array_equal(f, f1) and np.array_equal(c, c1)
    assert b.max() <= 3 * 8 * M.acc_term_bound(5, np.abs(logits).max()) and b[c > 0].min() >= 8 * M.acc_term_bound(5, 0.0)
    assert M.acc_term_bound(6, 2.0) == 14 * 2.0 ** -23 + 2.0 ** -19
    assert np.allclose(M.crop_bound(np.zeros((3, 1, 1)))[:, 0, 0], [8 * 255 * 2.0 ** -24 / s for s in STD], rtol=1e-15)


def test_footprints_and_their_grids():
    from emrt_amd.src.api import infer
    from emrt_amd.src.api import scene as S
    assert S.footprint((256, 256), (128, 128), 0.75) == ((341, 341), (171, 171))
    assert S.footprint((256, 256), (256, 128), 1.25) == ((205, 205), (205, 102))
    assert S.footprint((24, 16), (24, 12), 0.75) == ((32, 21), (32, 16))
    assert S.footprint((16, 16), (1, 1), 4.0) == ((4, 4), (1, 1))            # the stride is clamped to 1 from below ...
    assert S.footprint((10, 10), (10, 10), 0.8) == ((13, 13), (13, 13))      # ... and to the footprint from above
    assert [S.footprint((16, 16), (12, 12), s)[0][0] for s in M.SCALES] == [32, 20, 16, 10, 8]
    for crop, stride in (((32, 32), (24, 24)), ((24, 16), (13, 11))):
        assert S.footprint(crop, stride, 1.0) == (crop, stride)              # at s = 1: today's windows
        for s in (0.5, 0.75, 1.0, 1.5, 2.0):
            size, step, org = M.footprints(72, 88, crop, stride, s)
            assert S.footprint(crop, stride, s) == (size, step)
            assert org == [(a, b) for (a, b, _, _) in infer.window_grid(72, 88, size, step)]
            (s_, fh, fw, got), = S.footprint_grids(72, 88, crop, stride, (s,))
            assert (s_, fh, fw, got) == (s, size[1], size[0], org) and R.cover(72, 88, org, fh, fw).min() >= 1
    with pytest.raises(ValueError, match="footprint of 1 pixels"):
        S.footprint((5, 5), (5, 5), 4.0)                                     # 5 > 4 * 1: the library would refuse it
    with pytest.raises(ValueError, match="1..2048"):
        S.footprint((1024, 1024), (512, 512), 0.25)


# ---- the sixth library ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    from emrt_amd import build_ext
    build_ext.build(verbose=False)
    return build_ext


def test_sixth_library_exports_exactly_what_its_header_declares(built):
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.MST_HEADER)
    assert sorted(protos) == sorted(ENTRY + ("emrt_mst_last_error", "emrt_mst_version"))
    out = subprocess.run(["nm", "-D", "--defined-only", built.library("mstta").lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {n for n in exported if n.startswith("emrt_")} == set(protos)
    assert [len(protos[n][1]) for n in ENTRY] == [19, 15]
    assert [a for _, a in protos[ENTRY[1]][1]] == ["logits", "final", "count", "origins_yx", "n", "codes", "G", "C", "H", "W", "fh", "fw", "ch", "cw", "stream"]
    others = [_lib.parse_header(), _lib.parse_header(_lib.AUG_HEADER), _lib.parse_header(_lib.SMP_HEADER), _lib.parse_header(_lib.LOSS_HEADER),
              _lib.parse_header(_lib.TTA_HEADER)]
    assert [len(o) for o in others] == [109, 6, 4, 7, 4]                     # the five pinned headers are untouched
    assert not set(protos) & set().union(*others)
    assert _lib.MST_HEADER in built._headers()
    for path in (os.path.join(built.library("mstta").dir, "mstta_ext.hip"), os.path.join(built.CSRC, "window_variants.hpp")):
        text = open(path).read()
        assert "atomicAdd" not in text and "__hip_atomic" not in text and "scene_norm.hpp\"" in text and "float normalise_f32(" not in text, path
    assert "float normalise_f32(" in open(os.path.join(built.CSRC, "scene_norm.hpp")).read()


def test_loader_of_the_sixth_library(built, monkeypatch, tmp_path):
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_MST_LIB", None)
    T = _lib.mst_lib()
    assert T.query("emrt_mst_version") == 1 and T is _lib.mst_lib() and sorted(T.protos) == sorted(_lib.parse_header(_lib.MST_HEADER))
    assert T.last_error() == "" or isinstance(T.last_error(), str)
    monkeypatch.setitem(_lib.SIDE_LIBRARIES, "mstta", _lib.SIDE_LIBRARIES["mstta"]._replace(path=str(tmp_path / "nope.so")))
    monkeypatch.setattr(_lib, "_MST_LIB", None)
    with pytest.raises(_lib.EmrtHipError, match="not found"):
        _lib.mst_lib()


def _ints(values):
    arr = (ctypes.c_int * max(1, len(values)))(*values)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_entry_points_refuse_bad_arguments_before_any_launch(built, monkeypatch):
    """Against the real library, no GPU: every bad call returns non-zero with a message before anything touches a device (the device pointers
    are a made-up address and never dereferenced; a case that passed its checks would launch on them)."""
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_MST_LIB", None)
    T = _lib.mst_lib()
    p = ctypes.c_void_p(0x10000)
    norm = MEAN + [1.0 / s for s in STD]
    keep = []

    def args(org, codes):
        a, b = _ints([v for yx in org for v in yx]), _ints(codes)
        keep.extend([a, b])
        return a[1], b[1]

    def crop(match, org=((0, 0), (4, 8)), codes=(0, 1), n=None, G=None, H=24, W=28, fh=20, fw=20, ch=16, cw=16, scene=p, batch=p, null_org=False,
             null_codes=False):
        op, kp = args(org, codes)
        with pytest.raises(_lib.EmrtHipError, match=match) as e:
            T.call("emrt_mst_crop_windows_u8", scene, batch, None if null_org else op, len(org) if n is None else n, None if null_codes else kp,
                   len(codes) if G is None else G, H, W, fh, fw, ch, cw, *norm, None)
        assert "launch failed" not in str(e.value)

    def acc(match, org=((0, 0), (4, 8)), codes=(0, 1), n=None, G=None, C=6, H=24, W=28, fh=20, fw=20, ch=16, cw=16, logits=p, final=p, count=p,
            null_org=False, null_codes=False):
        op, kp = args(org, codes)
        with pytest.raises(_lib.EmrtHipError, match=match) as e:
            T.call("emrt_mst_window_accumulate", logits, final, count, None if null_org else op, len(org) if n is None else n,
                   None if null_codes else kp, len(codes) if G is None else G, C, H, W, fh, fw, ch, cw, None)
        assert "launch failed" not in str(e.value)

    crop("emrt_mst_crop_windows_u8: null pointer", scene=None)
    crop("null pointer", batch=None)
    crop("null pointer", null_org=True)
    crop("null pointer", null_codes=True)
    acc("emrt_mst_window_accumulate: null pointer", logits=None)
    acc("null pointer", final=None)
    acc("null pointer", count=None)
    acc("null pointer", null_org=True)
    acc("null pointer", null_codes=True)
    for call in (crop, acc):
        call("G must be 1..8", codes=(), G=0)
        call("G must be 1..8", codes=tuple(range(8)) + (0,), G=9)
        call("n \\* G <= 64", org=((0, 0),) * 9, codes=tuple(range(8)))                   # 72 images
        call("n \\* G <= 64", org=((0, 0),) * 33, codes=(0, 1))
        call("n \\* G <= 64", n=0)
        call("codes must be 0..7", codes=(0, 8))
        call("codes must be 0..7", codes=(-1,))
        call("a code is repeated", codes=(0, 1, 0))
        call("a transposing code \\(4..7\\) needs ch == cw", codes=(0, 4), ch=16, cw=12)
        call("a transposing code", codes=(7,), ch=12, cw=16)
        for edge in ("fh", "fw", "ch", "cw"):
            call("fh, fw, ch, cw must be 1..2048", **{edge: 0})
            call("fh, fw, ch, cw must be 1..2048", H=4096, W=4096, **{edge: 2049})
        call("differ by more than 4 times", H=80, W=80, fh=65)                             # f > 4 c
        call("differ by more than 4 times", H=80, W=80, fw=65)
        call("differ by more than 4 times", fh=3)                                          # c > 4 f
        call("differ by more than 4 times", fw=3)
        call("a footprint reaches outside the scene", org=((0, 0), (5, 8)))                # one row below the scene
        call("a footprint reaches outside the scene", org=((0, 9), (0, 0)))                # one column to the right
        call("a footprint reaches outside the scene", org=((-1, 0),))
        call("a footprint reaches outside the scene", H=19)                                # the scene is smaller than a footprint
        call("H and W must be positive", W=0)
    acc("C must be 1..256", C=0)
    acc("C must be 1..256", C=257)


# ---- host logic on the recording stand-ins ---------------------------------------------------------------------------------------------------
def _ints_of(ptr, n):
    arr = ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int))
    return [arr[i] for i in range(n)]


class FakeMstLib:
    """Recording stand-in for libemrt_hip_mstta.so: checks argument count and kinds against include/emrt_hip_mstta.h and logs.  Computes nothing.
    The two host arrays are read while the call runs, as the library reads them: hosts[k] = (origins [(y, x)], codes) of calls[k]."""

    def __init__(self):
        from emrt_amd import _lib
        self.protos = _lib.parse_header(_lib.MST_HEADER)
        self.calls, self.hosts = [], []

    def call(self, name, *args):
        spec = self.protos[name][1]
        assert len(args) == len(spec), "%s: %d args given, header declares %d" % (name, len(args), len(spec))
        for a, (t, an) in zip(args, spec):
            if t.endswith("*"):
                assert a is None or isinstance(a, (ctypes.c_void_p, int)), "%s.%s: bad pointer %r" % (name, an, a)
            elif t in ("float", "double"):
                assert isinstance(a, float), "%s.%s: expected a float, got %r" % (name, an, a)
            else:
                assert isinstance(a, int) and not isinstance(a, bool), "%s.%s (%s): expected int, got %r" % (name, an, t, a)
        named = dict(zip([an for _, an in spec], args))
        org = _ints_of(named["origins_yx"], 2 * named["n"])
        self.hosts.append((list(zip(org[0::2], org[1::2])), _ints_of(named["codes"], named["G"])))
        self.calls.append((name, args))


class _Model:
    """stands where the network stands: fp32 [n, ncls, h, w] logits for an fp32 [n, 3, h, w] batch, and a record of the calls"""

    def __init__(self, ncls):
        self.ncls, self.batches = ncls, []

    def eval(self):
        pass

    def __call__(self, x):
        self.batches.append(tuple(x.shape))
        return [torch.zeros(x.shape[0], self.ncls, x.shape[2], x.shape[3])]


def _raiser(what):
    def fn():
        raise AssertionError(what)
    return fn


@pytest.fixture()
def fakes(monkeypatch):
    from emrt_amd import _lib
    main, mst = fake_abi.install(), FakeMstLib()
    monkeypatch.setattr(_lib, "_MST_LIB", mst)
    monkeypatch.setattr(_lib, "tta_lib", _raiser("tta_scales loaded the fifth library"))
    yield main, mst
    fake_abi.uninstall()


def _predictor(ncls=6, crop=(64, 64), stride=(32, 32), **kw):
    from emrt_amd.src.api.scene import ScenePredictor
    from emrt_amd.src.utils import vis
    model = _Model(ncls)
    return model, ScenePredictor(model, ncls, crop, stride, vis.get_palette("Potsdam")[:ncls], MEAN, STD, **kw)


def _expected_launches(H, W, crop, stride, scales, G, max_batch):
    """[(fh, fw, [origins of one chunk])] in launch order: scales as given, footprints in grid order, max_batch // G per model call"""
    out = []
    for s in scales:
        (fw, fh), _, org = M.footprints(H, W, crop, stride, s)
        out += [(fh, fw, org[i:i + max_batch // G]) for i in range(0, len(org), max_batch // G)]
    return out


@pytest.mark.parametrize("mode", ["none", "hflip", "d4"])
def test_scene_with_scales_issues_the_two_launches_per_chunk_scale_by_scale(fakes, mode):
    from emrt_amd.src.api.scene import TTA_MODES
    main, mst = fakes
    codes = list(TTA_MODES[mode])
    G, scales = len(codes), (1.25, 0.75, 1.0)                   # the order given is the order run
    model, p = _predictor(max_batch=20, overlay=0.5, tta=mode, tta_scales=scales)
    assert p.tta_scales == scales
    scene = torch.zeros(100, 170, 3, dtype=torch.uint8)
    res = p(scene)
    want = _expected_launches(100, 170, (64, 64), (32, 32), scales, G, 20)
    assert [fh for fh, _, _ in want][0] == 51 and {fh for fh, _, _ in want} == {51, 85, 64}
    assert [n for n, _ in mst.calls] == list(ENTRY) * len(want)
    assert [n for n, _ in main.calls if n != "emrt_memset"] == ["emrt_scene_finish"]          # neither the plain crop nor the plain accumulation
    assert model.batches == [(len(chunk) * G, 3, 64, 64) for _, _, chunk in want]
    for k, (fh, fw, chunk) in enumerate(want):
        crop, acc = mst.calls[2 * k][1], mst.calls[2 * k + 1][1]
        assert crop[0].value == scene.data_ptr() and crop[3] == len(chunk) and mst.hosts[2 * k] == (chunk, codes)
        assert crop[5:12] == (G, 100, 170, fh, fw, 64, 64) and list(crop[12:18]) == MEAN + [1.0 / s for s in STD]
        assert acc[4] == len(chunk) and mst.hosts[2 * k + 1] == (chunk, codes) and acc[0].value != crop[1].value
        assert acc[6:14] == (G, 6, 100, 170, fh, fw, 64, 64)
        assert acc[1].value == mst.calls[1][1][1].value and acc[2].value == mst.calls[1][1][2].value          # one pair of sums for all scales
    fin = [a for n, a in main.calls if n == "emrt_scene_finish"][0]
    acc = mst.calls[-1][1]
    assert fin[0].value == acc[1].value and fin[1].value == acc[2].value and fin[9:13] == (1, 6, 100, 170)
    assert fin[3].value == scene.data_ptr() and res.index.shape == (100, 170)


def test_evaluator_with_scales_accumulates_through_the_sixth_library(fakes, tmp_path):
    from emrt_amd.src.api.scene import SceneEvaluator
    from emrt_amd.src.datasets import SceneBank
    main, mst = fakes
    sizes = [(96, 96), (130, 200)]
    write_scene_tree(str(tmp_path), sizes, sub=VAL_SUB)
    bank = SceneBank(str(tmp_path), "cpu", 0, sub=VAL_SUB, shift_on_upload=True)
    model = _Model(6)
    ev = SceneEvaluator(model, bank, 6, (64, 64), (48, 48), MEAN, STD, max_batch=16, tta="flips", tta_scales=[0.75, 1.0])
    assert main.calls == [] and mst.calls == [] and ev.tta_scales == (0.75, 1.0)
    ev.evaluate()
    assert [n for n, _ in main.calls if n != "emrt_memset"] == ["emrt_window_normalise", "emrt_argmax_nchw", "emrt_segmentation_areas"] * 2
    want_batches, k = [], 0
    for H, W in sizes:
        for fh, fw, chunk in _expected_launches(H, W, (64, 64), (48, 48), (0.75, 1.0), 4, 16):
            crop, acc = mst.calls[k][1], mst.calls[k + 1][1]
            assert (mst.calls[k][0], mst.calls[k + 1][0]) == ENTRY and len(chunk) <= 4
            assert crop[3] == len(chunk) == acc[4] and crop[5:12] == (4, H, W, fh, fw, 64, 64) and acc[6:14] == (4, 6, H, W, fh, fw, 64, 64)
            assert mst.hosts[k] == mst.hosts[k + 1] == (chunk, [0, 1, 2, 3])
            want_batches.append((len(chunk) * 4, 3, 64, 64))
            k += 2
    assert k == len(mst.calls) and model.batches == want_batches
    norms = [a for n, a in main.calls if n == "emrt_window_normalise"]
    assert norms[1][0].value == mst.calls[-1][1][1].value and norms[1][1].value == mst.calls[-1][1][2].value


def test_no_scales_takes_todays_paths_and_never_touches_the_sixth_library(monkeypatch, tmp_path):
    from emrt_amd import _lib
    from emrt_amd.src.api.scene import SceneEvaluator
    from emrt_amd.src.datasets import SceneBank
    from tests.test_tta_cpu import FakeTtaLib
    main, tta = fake_abi.install(), FakeTtaLib()
    try:
        monkeypatch.setattr(_lib, "_TTA_LIB", tta)
        monkeypatch.setattr(_lib, "_MST_LIB", None)
        monkeypatch.setattr(_lib, "mst_lib", _raiser("tta_scales=None loaded the sixth library"))
        scene = torch.zeros(100, 170, 3, dtype=torch.uint8)
        for mode, per_chunk, chunks in (("none", ["emrt_scene_crop_windows_u8", "emrt_window_accumulate"], 4), ("flips", [], 0)):
            logs = []
            for kw in ({}, {"tta_scales": None}):
                del main.calls[:], tta.calls[:]
                model, p = _predictor(max_batch=4, tta=mode, **kw)
                p(scene)
                p.predict_tiles(torch.zeros(5, 64, 64, 3, dtype=torch.uint8))
                logs.append(([n for n, _ in main.calls], [n for n, _ in tta.calls], model.batches))
            assert logs[0] == logs[1]
            assert [n for n in logs[0][0] if n != "emrt_memset"][:2 * chunks + 1] == per_chunk * chunks + ["emrt_scene_finish"]
            assert (logs[0][1] == []) == (mode == "none")
        write_scene_tree(str(tmp_path), [(64, 80)], sub=VAL_SUB)
        bank = SceneBank(str(tmp_path), "cpu", 0, sub=VAL_SUB, shift_on_upload=True)
        del main.calls[:]
        SceneEvaluator(_Model(6), bank, 6, (64, 64), (48, 48), MEAN, STD, tta_scales=None).evaluate()
        assert [n for n, _ in main.calls if n != "emrt_memset"] == ["emrt_scene_crop_windows_u8", "emrt_window_accumulate", "emrt_window_normalise",
                                                                    "emrt_argmax_nchw", "emrt_segmentation_areas"]
    finally:
        fake_abi.uninstall()


def test_value_errors_of_the_tta_scales_argument(fakes, tmp_path):
    from emrt_amd.src.api.scene import SceneEvaluator, check_tta_scales
    from emrt_amd.src.datasets import SceneBank
    main, mst = fakes
    for bad in ((), [], 0.75, "0.75", object(), ("a",)):
        with pytest.raises(ValueError, match="non-empty sequence of scales"):
            _predictor(tta_scales=bad)
    for bad in ((0.2,), (1.0, 4.5), (float("nan"),), (-1.0,)):
        with pytest.raises(ValueError, match=r"must lie in \[0.25, 4\]"):
            _predictor(tta_scales=bad)
    with pytest.raises(ValueError, match="repeats a scale"):
        _predictor(tta_scales=(0.75, 1.0, 0.75))
    with pytest.raises(ValueError, match="tta_scales cannot be combined with scales"):
        _predictor(tta_scales=(0.75, 1.0), scales=(0.75, 1.0))
    with pytest.raises(ValueError, match="max_batch >= 8, got 7"):
        _predictor(tta_scales=(0.75,), tta="d4", max_batch=7)
    with pytest.raises(ValueError, match="needs a square crop"):
        _predictor(tta_scales=(0.75,), tta="d4", crop=(64, 48))
    assert check_tta_scales(None, (1.0,)) is None and check_tta_scales([0.25, 4, 1], None) == (0.25, 4.0, 1.0)
    assert check_tta_scales(np.asarray([0.5, 2.0]), None) == (0.5, 2.0)
    _, p = _predictor(tta_scales=(0.25, 4.0), tta="d4", max_batch=8)        # every mode, the ends of the range
    assert p.tta_scales == (0.25, 4.0) and p.codes == tuple(range(8))
    # a scene smaller than a footprint: refused per scene, naming the scale and the scene; nothing is launched
    _, p = _predictor(tta_scales=(1.0, 0.5))
    with pytest.raises(ValueError, match=r"scene 100x127 \(h x w\) is smaller than the 128x128 footprint of the 64x64 crop at scale 0.5"):
        p(torch.zeros(100, 127, 3, dtype=torch.uint8))
    _, p = _predictor(tta_scales=(2.0,))
    p(torch.zeros(40, 50, 3, dtype=torch.uint8))                             # smaller than the crop, not than the 32 x 32 footprint
    assert len(mst.calls) == 2 and mst.hosts[0][0] == M.footprints(40, 50, (64, 64), (32, 32), 2.0)[2] and len(mst.hosts[0][0]) == 6
    assert mst.calls[0][1][5:12] == (1, 40, 50, 32, 32, 64, 64)
    del mst.calls[:], main.calls[:]
    with pytest.raises(ValueError, match="predict_tiles does not take tta_scales"):
        p.predict_tiles(torch.zeros(5, 64, 64, 3, dtype=torch.uint8))
    write_scene_tree(str(tmp_path), [(96, 96), (64, 80)], sub=VAL_SUB)
    bank = SceneBank(str(tmp_path), "cpu", 0, sub=VAL_SUB, shift_on_upload=True)
    with pytest.raises(ValueError, match=r"scene 1 \(%s\) 64x80 \(h x w\) is smaller than the 85x85 footprint of the 64x64 crop at scale 0.75" % bank.names[1]):
        SceneEvaluator(_Model(6), bank, 6, (64, 64), (48, 48), MEAN, STD, tta_scales=(1.0, 0.75))
    for kw, match in (({"tta_scales": ()}, "non-empty sequence"), ({"tta_scales": (5.0,)}, "must lie in"), ({"tta_scales": (1.0, 1.0)}, "repeats"),
                      ({"tta_scales": (1.0,), "scales": (1.0,)}, "cannot be combined with scales")):
        with pytest.raises(ValueError, match=match):
            SceneEvaluator(_Model(6), bank, 6, (64, 64), (48, 48), MEAN, STD, **kw)
    assert main.calls == [] and mst.calls == []


# ---- the command lines -----------------------------------------------------------------------------------------------------------------------
def test_predict_and_val_parse_the_tta_scales_flag(capsys):
    from emrt_amd import predict, val
    from emrt_amd.config import get_config
    from emrt_amd.src.api.scene import refuse_scales_with_config
    assert predict.parse_args([]).tta_scales is None and val.parse_args([]).tta_scales is None
    assert predict.parse_args(["--tta_scales", "0.75", "1.0", "1.25"]).tta_scales == [0.75, 1.0, 1.25]
    a = predict.parse_args(["--tta", "d4", "--tta_scales", "0.5", "2"])
    assert a.tta == "d4" and a.tta_scales == [0.5, 2.0]
    a = val.parse_args(["--data", "scenes", "--tta", "flips", "--tta_scales", "0.75", "1"])
    assert a.tta == "flips" and a.tta_scales == [0.75, 1.0]
    for mod, argv, text in ((predict, ["--tta_scales"], "expected at least one argument"),
                            (predict, ["--tta_scales", "x"], "invalid float value"),
                            (predict, ["--tta_scales", "0.1"], "must lie in [0.25, 4]"),
                            (predict, ["--tta_scales", "1", "1"], "repeats a scale"),
                            (predict, ["--tta_scales", "0.75", "--multi_scales"], "--tta_scales cannot be combined with --multi_scales"),
                            (val, ["--tta_scales", "0.75"], "--tta_scales needs --data scenes"),
                            (val, ["--data", "dataset", "--tta_scales", "0.75"], "--tta_scales needs --data scenes"),
                            (val, ["--data", "tiles.npz", "--tta_scales", "0.75"], "--data tiles.npz is not"),
                            (val, ["--data", "scenes", "--tta_scales", "8"], "must lie in [0.25, 4]"),
                            (val, ["--data", "scenes", "--tta_scales", "0.75", "--multi_scales"], "--tta_scales cannot be combined with --multi_scales")):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, (argv, text)
    cfg = get_config()
    refuse_scales_with_config(predict.parse_args(["--tta_scales", "0.75"]), cfg)              # VAL.MULTI_SCALES_VAL is off by default
    cfg.defrost()
    cfg.VAL.MULTI_SCALES_VAL = True
    refuse_scales_with_config(predict.parse_args([]), cfg)
    for args in (predict.parse_args(["--tta_scales", "0.75"]), val.parse_args(["--data", "scenes", "--tta_scales", "0.75"])):
        with pytest.raises(SystemExit) as e:
            refuse_scales_with_config(args, cfg)
        assert e.value.code == 2 and "cannot be combined with VAL.MULTI_SCALES_VAL" in capsys.readouterr().err


def test_val_passes_the_scales_to_the_evaluator(tmp_path):
    from emrt_amd import val
    from emrt_amd.config import get_config
    fake_abi.install()
    try:
        write_scene_tree(str(tmp_path), [(96, 96)], sub=VAL_SUB)
        cfg = get_config()
        cfg.DATA.DATA_PATH = str(tmp_path)
        cfg.VAL.CROP_SIZE, cfg.VAL.STRIDE_SIZE = [64, 64], [48, 48]
        ev = val.scene_evaluator(_Model(6), cfg, "cpu", tta="d4", max_batch=16, tta_scales=[0.75, 1.0])
        assert ev.tta == "d4" and ev.tta_scales == (0.75, 1.0) and ev.max_batch == 16
        assert val.scene_evaluator(_Model(6), cfg, "cpu").tta_scales is None
    finally:
        fake_abi.uninstall()


# ---- what the GPU cases can decide, judged from the reference alone ----------------------------------------------------------------------------
def test_the_gpu_cases_leave_at_most_one_percent_of_the_pixels_undecided(tmp_path):
    """Class indices are compared wherever the reference's two largest sums are further apart than twice the per-pixel bound; this is the share
    left out, for the exact seeds and shapes of tests/test_gpu_ms_tta.py."""
    H, W = M.ACC_MAP
    worst = 0.0
    for C in M.ACC_CLASSES:
        if C < 2:
            continue                                          # one class: nothing to decide
        for s in M.SCALES:
            for mode in M.ACC_MODES:
                org, fh, fw, logits, final0, count0 = M.acc_case(C, s, mode)
                final, _, bound = M.accumulate_ms(logits, org, M.MODES[mode], H, W, fh, fw, final=np.zeros((C, H, W)))
                share = M.undecided(final, bound)
                worst = max(worst, share)
                assert share <= 0.01, (C, s, mode, share)
    arrays = write_scene_tree(str(tmp_path), M.PIPE_SIZES, sub=VAL_SUB, seed=M.PIPE_SEED)
    mix, ramp = M.stub_params(equivariant=False)
    for img, _ in arrays:
        for mode in M.PIPE_MODES:
            final, count, bound = M.pipeline_reference(img, M.PIPE_CROP, M.PIPE_STRIDE, M.PIPE_SCALES, M.MODES[mode], M.PIPE_MAX_BATCH,
                                                       lambda b: M.stub_logits(b, mix, ramp))
            share = M.undecided(final, bound)
            worst = max(worst, share)
            assert count.min() >= len(M.PIPE_SCALES) * len(M.MODES[mode]) and share <= 0.01, (img.shape, mode, share)
    print("largest share of undecided pixels over the GPU cases: %.3f %%" % (100 * worst))
