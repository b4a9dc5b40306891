"""CPU: flip and rotation test-time augmentation of whole-scene inference -- the numpy restatement's own consistency
(tests/tta_reference.py), the fifth library's header, build, loader and host-side refusals, the launches ScenePredictor / SceneEvaluator issue
under every mode (on recording stand-ins for the first and the fifth library: nothing is computed) and the two command lines' flags.  The
kernels themselves are held to the restatement in tests/test_gpu_tta.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import fake_abi
from tests import tta_reference as R
from tests.test_scene_sampler_cpu import write_scene_tree

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
VAL_SUB = ("val_images", "val_labels")
ENTRY = ("emrt_tta_crop_windows_u8", "emrt_tta_window_accumulate")


# ---- the reference itself ------------------------------------------------------------------------------------------------------------------
def test_reference_variants_and_inverses():
    a = np.arange(2 * 5 * 5, dtype=np.float64).reshape(2, 5, 5) ** 1.5          # no symmetry: every variant differs from every other
    seen = []
    for code in range(8):
        v = R.variant(a, code)
        assert np.array_equal(R.inverse(v, code), a), code
        assert not any(np.array_equal(v, s) for s in seen), code
        seen.append(v)
    rot = lambda k: np.rot90(a, k, axes=(-2, -1))
    assert np.array_equal(R.variant(a, 0), a) and np.array_equal(R.variant(a, 1), a[..., ::-1]) and np.array_equal(R.variant(a, 2), a[..., ::-1, :])
    assert np.array_equal(R.variant(a, 3), rot(2)) and np.array_equal(R.variant(a, 4), np.swapaxes(a, -1, -2))
    assert np.array_equal(R.variant(a, 5), rot(1)) and np.array_equal(R.variant(a, 6), rot(-1))
    assert np.array_equal(R.variant(a, 7), rot(2).swapaxes(-1, -2))               # the anti-transpose
    b = np.arange(3 * 4 * 6, dtype=np.float64).reshape(3, 4, 6)                    # a rectangle under the flips
    for code in range(4):
        assert R.variant(b, code).shape == b.shape and np.array_equal(R.inverse(R.variant(b, code), code), b)
    assert R.MODES == {"none": [0], "hflip": [0, 1], "flips": [0, 1, 2, 3], "d4": list(range(8))}


def test_reference_sums_are_mean_probabilities_and_counts_are_g_times_cover():
    rng = np.random.RandomState(5)
    H, W, ch, cw, C = 9, 11, 4, 4, 3
    org = [(0, 0), (2, 3), (5, 7), (2, 3)]
    codes = R.MODES["d4"]
    logits = rng.randn(len(org) * 8, C, ch, cw)
    final, count = R.accumulate(logits, org, codes, H, W)
    cov = R.cover(H, W, org, ch, cw)
    assert np.array_equal(count, 8.0 * cov) and cov.max() == 3 and cov.min() == 0
    assert np.allclose(final.sum(0), count, rtol=0, atol=1e-12)                    # every term is a probability vector
    # an exactly equivariant "model" (the logits are a pixelwise function of the variant): every variant votes the same
    scene = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    batch = R.crop_variants(scene, org, codes, ch, cw, MEAN, STD)
    assert batch.shape == (32, 3, 4, 4) and np.array_equal(R.inverse(batch[8 + 5], 5), batch[8])
    mix = rng.randn(C, 3)
    eq, _ = R.accumulate(np.einsum("kc,nchw->nkhw", mix, batch), org, codes, H, W)
    one, _ = R.accumulate(np.einsum("kc,nchw->nkhw", mix, batch[::8]), org, [0], H, W)
    assert np.allclose(eq, 8.0 * one, rtol=0, atol=1e-12)
    f2, c2 = R.accumulate(logits, org, codes, H, W, final=np.ones((C, H, W)), count=np.full((H, W), 2.0))
    assert np.allclose(f2, final + 1.0, rtol=0, atol=1e-12) and np.array_equal(c2, count + 2.0)
    assert R.bound(4, 8, 6) == 4 * 8 * 14 * 2.0 ** -23


# ---- the fifth library ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    from emrt_amd import build_ext
    build_ext.build(verbose=False)
    return build_ext


def test_fifth_library_exports_exactly_what_its_header_declares(built):
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.TTA_HEADER)
    assert sorted(protos) == sorted(ENTRY + ("emrt_tta_last_error", "emrt_tta_version"))
    out = subprocess.run(["nm", "-D", "--defined-only", built.library("tta").lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {n for n in exported if n.startswith("emrt_")} == set(protos)
    others = [_lib.parse_header(), _lib.parse_header(_lib.AUG_HEADER), _lib.parse_header(_lib.SMP_HEADER), _lib.parse_header(_lib.LOSS_HEADER)]
    assert [len(o) for o in others] == [109, 6, 4, 7]                        # the four pinned headers are untouched
    assert not set(protos) & set().union(*others)
    assert [len(protos[n][1]) for n in ENTRY] == [17, 13]
    assert _lib.TTA_HEADER in built._headers() and os.path.join(built.CSRC, "scene_norm.hpp") in built._headers()


def test_normalisation_is_written_once():
    """normalise_u8 lives in csrc/scene_norm.hpp; scene.hip, tta_ext.hip and window_variants.hpp include it and none restates it"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "emrt_amd", "csrc")
    assert "float normalise_u8(" in open(os.path.join(csrc, "scene_norm.hpp")).read()
    for f in ("scene.hip", os.path.join("tta_ext", "tta_ext.hip"), "window_variants.hpp"):
        text = open(os.path.join(csrc, f)).read()
        assert "scene_norm.hpp\"" in text and "float normalise_u8(" not in text and "float normalise_f32(" not in text, f
        assert f == "scene.hip" or ("atomicAdd" not in text and "__hip_atomic" not in text), f


def test_what_the_two_window_libraries_share_is_written_once(built):
    """The variant codes with their refusals and decoding, the tile constants and the box tiles live in csrc/window_variants.hpp (an input of
    every object); tta_ext.hip and mstta_ext.hip include it and neither restates any of it.  (The kernels' write-out loop and softmax are still
    each file's own: the same text in both, see the header's comment.)"""
    shared = os.path.join(built.CSRC, "window_variants.hpp")
    assert shared in built._headers()
    owned = ("struct VariantCodes", '"G must be 1..8"', '"n >= 1 and n * G <= 64"', '"codes must be 0..7"', '"a code is repeated"',
             '"a transposing code (4..7) needs ch == cw"', "Variant decode_variant(", "struct BoxTiles", "long long fill_box_tiles(", "x_lo", "constexpr int CT =",
             "constexpr int CROW =", "constexpr int CPLANE =", "constexpr int AT =", "constexpr int ACH =", "static_assert(EMRT_TTA_MAX_VARIANTS == EMRT_MST_MAX_VARIANTS")
    text = open(shared).read()
    for s in owned:
        assert s in text, s
    for name in ("tta", "mstta"):
        row = built.library(name)
        text = open(os.path.join(row.dir, row.sources[0])).read()
        assert "../window_variants.hpp\"" in text, name
        for s in owned + ("struct TtaCodes", "struct MstCodes", "struct TtaTiles", "struct MstTiles"):
            assert s not in text, (name, s)
        for s in ("VariantCodes k", "BoxTiles tl", "fill_box_tiles(", "check_variant_counts(", "fill_variant_codes(", "decode_variant("):
            assert s in text, (name, s)


def test_loader_of_the_fifth_library(built, monkeypatch, tmp_path):
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_TTA_LIB", None)
    T = _lib.tta_lib()
    assert T.query("emrt_tta_version") == 1 and T is _lib.tta_lib() and sorted(T.protos) == sorted(_lib.parse_header(_lib.TTA_HEADER))
    monkeypatch.setitem(_lib.SIDE_LIBRARIES, "tta", _lib.SIDE_LIBRARIES["tta"]._replace(path=str(tmp_path / "nope.so")))
    monkeypatch.setattr(_lib, "_TTA_LIB", None)
    with pytest.raises(_lib.EmrtHipError, match="not found"):
        _lib.tta_lib()


def _ints(values):
    arr = (ctypes.c_int * max(1, len(values)))(*values)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_entry_points_refuse_bad_arguments_before_any_launch(built, monkeypatch):
    """Against the real library, no GPU: every bad call returns non-zero with a message before anything touches a device (the device pointers
    are a made-up address and never dereferenced; a case that passed its checks would launch on them)."""
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_TTA_LIB", None)
    T = _lib.tta_lib()
    p = ctypes.c_void_p(0x10000)
    norm = MEAN + [1.0 / s for s in STD]
    keep = []

    def args(org, codes):
        a, b = _ints([v for yx in org for v in yx]), _ints(codes)
        keep.extend([a, b])
        return a[1], b[1]

    def crop(match, org=((0, 0), (4, 8)), codes=(0, 1), n=None, G=None, H=20, W=24, ch=16, cw=16, scene=p, batch=p, null_org=False, null_codes=False):
        op, kp = args(org, codes)
        with pytest.raises(_lib.EmrtHipError, match=match) as e:
            T.call("emrt_tta_crop_windows_u8", scene, batch, None if null_org else op, len(org) if n is None else n, None if null_codes else kp,
                   len(codes) if G is None else G, H, W, ch, cw, *norm, None)
        assert "launch failed" not in str(e.value)

    def acc(match, org=((0, 0), (4, 8)), codes=(0, 1), n=None, G=None, C=6, H=20, W=24, ch=16, cw=16, logits=p, final=p, count=p, null_org=False,
            null_codes=False):
        op, kp = args(org, codes)
        with pytest.raises(_lib.EmrtHipError, match=match) as e:
            T.call("emrt_tta_window_accumulate", logits, final, count, None if null_org else op, len(org) if n is None else n,
                   None if null_codes else kp, len(codes) if G is None else G, C, H, W, ch, cw, None)
        assert "launch failed" not in str(e.value)

    crop("emrt_tta_crop_windows_u8: null pointer", scene=None)
    crop("null pointer", batch=None)
    crop("null pointer", null_org=True)
    crop("null pointer", null_codes=True)
    acc("emrt_tta_window_accumulate: null pointer", logits=None)
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
        call("1..64 windows inside the image", org=((0, 0), (5, 8)))                       # one row below the scene
        call("1..64 windows inside the image", org=((0, 9), (0, 0)))                       # one column to the right
        call("1..64 windows inside the image", org=((-1, 0),))
        call("H, W, ch, cw must be positive", ch=0)
        call("H, W, ch, cw must be positive", W=0)
    acc("C must be 1..256", C=0)
    acc("C must be 1..256", C=257)


# ---- host logic on the recording stand-ins ---------------------------------------------------------------------------------------------------
def _ints_of(ptr, n):
    arr = ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int))
    return [arr[i] for i in range(n)]


class FakeTtaLib:
    """Recording stand-in for libemrt_hip_tta.so: checks argument count and kinds against include/emrt_hip_tta.h and logs.  Computes nothing.
    The two host arrays are read while the call runs, as the library reads them: hosts[k] = (origins [(y, x)], codes) of calls[k]."""

    def __init__(self):
        from emrt_amd import _lib
        self.protos = _lib.parse_header(_lib.TTA_HEADER)
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


@pytest.fixture()
def fakes(monkeypatch):
    from emrt_amd import _lib
    main, tta = fake_abi.install(), FakeTtaLib()
    monkeypatch.setattr(_lib, "_TTA_LIB", tta)
    yield main, tta
    fake_abi.uninstall()


def _predictor(ncls=6, crop=(64, 64), stride=(32, 32), **kw):
    from emrt_amd.src.api.scene import ScenePredictor
    from emrt_amd.src.utils import vis
    model = _Model(ncls)
    return model, ScenePredictor(model, ncls, crop, stride, vis.get_palette("Potsdam")[:ncls], MEAN, STD, **kw)


@pytest.mark.parametrize("mode", ["hflip", "flips", "d4"])
def test_scene_under_tta_issues_the_two_launches_per_chunk_of_max_batch_over_g(fakes, mode):
    from emrt_amd.src.api import infer
    from emrt_amd.src.api.scene import TTA_MODES
    main, tta = fakes
    codes = list(TTA_MODES[mode])
    assert codes == R.MODES[mode]
    G = len(codes)
    model, p = _predictor(max_batch=20, overlay=0.5, tta=mode)
    scene = torch.zeros(100, 170, 3, dtype=torch.uint8)
    res = p(scene)
    wins = infer.window_grid(100, 170, (64, 64), (32, 32))
    per = 20 // G                                           # 10, 5, 2 windows per model call
    chunks = [wins[i:i + per] for i in range(0, len(wins), per)]
    assert [n for n, _ in tta.calls] == list(ENTRY) * len(chunks)
    assert [n for n, _ in main.calls if n != "emrt_memset"] == ["emrt_scene_finish"]          # neither the plain crop nor the plain accumulation
    assert model.batches == [(len(c) * G, 3, 64, 64) for c in chunks]
    for k, chunk in enumerate(chunks):
        crop, acc = tta.calls[2 * k][1], tta.calls[2 * k + 1][1]
        want = [(a, b) for (a, b, _, _) in chunk]
        assert crop[0].value == scene.data_ptr() and crop[3] == len(chunk) and tta.hosts[2 * k] == (want, codes)
        assert crop[5:10] == (G, 100, 170, 64, 64) and list(crop[10:16]) == MEAN + [1.0 / s for s in STD]
        assert acc[4] == len(chunk) and tta.hosts[2 * k + 1] == (want, codes) and acc[0].value != crop[1].value
        assert acc[6:12] == (G, 6, 100, 170, 64, 64)
    fin = [a for n, a in main.calls if n == "emrt_scene_finish"][0]
    acc = tta.calls[-1][1]
    assert fin[0].value == acc[1].value and fin[1].value == acc[2].value and fin[9:13] == (1, 6, 100, 170)      # the sums and counts just made
    assert fin[3].value == scene.data_ptr() and res.index.shape == (100, 170)


def test_tta_none_issues_todays_launches_and_never_touches_the_fifth_library(fakes, monkeypatch, tmp_path):
    from emrt_amd import _lib
    from emrt_amd.src.api.scene import SceneEvaluator
    from emrt_amd.src.datasets import SceneBank
    main, tta = fakes
    monkeypatch.setattr(_lib, "_TTA_LIB", None)
    monkeypatch.setattr(_lib, "tta_lib", lambda: (_ for _ in ()).throw(AssertionError("tta='none' loaded the fifth library")))
    scene = torch.zeros(100, 170, 3, dtype=torch.uint8)
    logs = []
    for kw in ({}, {"tta": "none"}):
        del main.calls[:]
        model, p = _predictor(max_batch=4, **kw)
        p(scene)
        p.predict_tiles(torch.zeros(5, 64, 64, 3, dtype=torch.uint8))
        logs.append(([n for n, _ in main.calls], model.batches))
    assert logs[0] == logs[1]
    names = [n for n in logs[0][0] if n != "emrt_memset"]
    assert names == ["emrt_scene_crop_windows_u8", "emrt_window_accumulate"] * 4 + ["emrt_scene_finish"] + ["emrt_scene_crop_windows_u8", "emrt_scene_finish"] * 2
    write_scene_tree(str(tmp_path), [(64, 80)], sub=VAL_SUB)
    bank = SceneBank(str(tmp_path), "cpu", 0, sub=VAL_SUB, shift_on_upload=True)
    del main.calls[:]
    SceneEvaluator(_Model(6), bank, 6, (64, 64), (48, 48), MEAN, STD, tta="none").evaluate()
    assert [n for n, _ in main.calls if n != "emrt_memset"] == ["emrt_scene_crop_windows_u8", "emrt_window_accumulate", "emrt_window_normalise",
                                                                "emrt_argmax_nchw", "emrt_segmentation_areas"]
    assert tta.calls == []


def test_evaluator_under_tta_accumulates_through_the_fifth_library(fakes, tmp_path):
    from emrt_amd.src.api import infer
    from emrt_amd.src.api.scene import SceneEvaluator
    from emrt_amd.src.datasets import SceneBank
    main, tta = fakes
    sizes = [(64, 64), (130, 200)]
    write_scene_tree(str(tmp_path), sizes, sub=VAL_SUB)
    bank = SceneBank(str(tmp_path), "cpu", 0, sub=VAL_SUB, shift_on_upload=True)
    model = _Model(6)
    ev = SceneEvaluator(model, bank, 6, (64, 64), (48, 48), MEAN, STD, max_batch=16, tta="flips")
    assert main.calls == [] and tta.calls == []
    ev.evaluate()
    names = [n for n, _ in main.calls if n != "emrt_memset"]
    assert names == ["emrt_window_normalise", "emrt_argmax_nchw", "emrt_segmentation_areas"] * 2
    want_batches, k = [], 0
    for H, W in sizes:
        wins = infer.window_grid(H, W, (64, 64), (48, 48))
        for i in range(0, len(wins), 4):                    # 16 // 4 windows per call
            chunk = wins[i:i + 4]
            crop, acc = tta.calls[k][1], tta.calls[k + 1][1]
            assert (tta.calls[k][0], tta.calls[k + 1][0]) == ENTRY
            assert crop[3] == len(chunk) == acc[4] and crop[5:10] == (4, H, W, 64, 64) and acc[6:12] == (4, 6, H, W, 64, 64)
            assert tta.hosts[k] == tta.hosts[k + 1] == ([(a, b) for (a, b, _, _) in chunk], [0, 1, 2, 3])
            want_batches.append((len(chunk) * 4, 3, 64, 64))
            k += 2
    assert k == len(tta.calls) and model.batches == want_batches
    norms = [a for n, a in main.calls if n == "emrt_window_normalise"]
    assert norms[1][0].value == tta.calls[-1][1][1].value and norms[1][1].value == tta.calls[-1][1][2].value


def test_predict_tiles_under_tta_treats_each_chunk_as_one_tall_scene(fakes):
    main, tta = fakes
    model, p = _predictor(max_batch=9, tta="flips", overlay=0.25)
    tiles = torch.zeros(5, 64, 64, 3, dtype=torch.uint8)
    res = p.predict_tiles(tiles)
    assert model.batches == [(8, 3, 64, 64), (8, 3, 64, 64), (4, 3, 64, 64)]          # 9 // 4 = 2 tiles per call
    assert [n for n, _ in tta.calls] == list(ENTRY) * 3
    fins = [a for n, a in main.calls if n == "emrt_scene_finish"]
    assert [n for n, _ in main.calls if n != "emrt_memset"] == ["emrt_scene_finish"] * 3
    for k, (j0, m) in enumerate(((0, 2), (2, 2), (4, 1))):
        crop, acc, fin = tta.calls[2 * k][1], tta.calls[2 * k + 1][1], fins[k]
        assert crop[0].value == tiles[j0].data_ptr() and crop[3] == m and crop[5:10] == (4, m * 64, 64, 64, 64)
        assert tta.hosts[2 * k] == tta.hosts[2 * k + 1] == ([(j * 64, 0) for j in range(m)], [0, 1, 2, 3])
        assert acc[6:12] == (4, 6, m * 64, 64, 64, 64)
        assert fin[0].value == acc[1].value and fin[1].value == acc[2].value and fin[9:13] == (1, 6, m * 64, 64)
        assert fin[3].value == tiles[j0].data_ptr() and fin[4] == 0.25
        assert fin[5].value == res.index[j0].data_ptr() and fin[6].value == res.color[j0].data_ptr() and fin[7].value == res.overlay[j0].data_ptr()
        assert fin[8].value == res.areas.data_ptr()
    assert res.index.shape == (5, 64, 64)


def test_value_errors_of_the_tta_argument(fakes, tmp_path):
    from emrt_amd.src.api.scene import SceneEvaluator, check_tta
    from emrt_amd.src.datasets import SceneBank
    main, tta = fakes
    with pytest.raises(ValueError, match="tta must be one of none, hflip, flips, d4"):
        _predictor(tta="rot90")
    with pytest.raises(ValueError, match="needs a square crop, got 64x48"):
        _predictor(crop=(64, 48), tta="d4")
    _predictor(crop=(64, 48), tta="flips")                  # the flips take any rectangle
    with pytest.raises(ValueError, match="max_batch >= 8, got 7"):
        _predictor(max_batch=7, tta="d4")
    _predictor(max_batch=8, tta="d4")
    with pytest.raises(ValueError, match="max_batch >= 2, got 1"):
        _predictor(max_batch=1, tta="hflip")
    with pytest.raises(ValueError, match="cannot be combined with scales"):
        _predictor(scales=(0.75, 1.0), tta="hflip")
    _predictor(scales=(0.75, 1.0), tta="none")
    assert check_tta("none", (64, 48), 1, (1.0,)) == (0,) and check_tta("d4", (64, 64), 8, None) == tuple(range(8))
    write_scene_tree(str(tmp_path), [(64, 80)], sub=VAL_SUB)
    bank = SceneBank(str(tmp_path), "cpu", 0, sub=VAL_SUB, shift_on_upload=True)
    for kw, match in (({"tta": "d4", "max_batch": 4}, "max_batch >= 8"), ({"tta": "flips", "scales": (1.0,)}, "cannot be combined with scales"),
                      ({"tta": "all"}, "tta must be one of")):
        with pytest.raises(ValueError, match=match):
            SceneEvaluator(_Model(6), bank, 6, (64, 64), (48, 48), MEAN, STD, **kw)
    with pytest.raises(ValueError, match="needs a square crop"):
        SceneEvaluator(_Model(6), bank, 6, (64, 48), (48, 48), MEAN, STD, tta="d4")
    assert main.calls == [] and tta.calls == []


# ---- the command lines -----------------------------------------------------------------------------------------------------------------------
def test_predict_and_val_parse_the_tta_flag(capsys):
    from emrt_amd import predict, val
    assert predict.parse_args([]).tta == "none" and val.parse_args([]).tta == "none"
    for mode in ("none", "hflip", "flips", "d4"):
        assert predict.parse_args(["--tta", mode]).tta == mode
        assert val.parse_args(["--data", "scenes", "--tta", mode]).tta == mode
    assert val.parse_args(["--data", "dataset", "--tta", "none"]).tta == "none"
    for mod, argv, text in ((predict, ["--tta", "rot"], "invalid choice"),
                            (predict, ["--tta", "d4", "--multi_scales"], "cannot be combined with --multi_scales"),
                            (val, ["--tta", "d4"], "--tta d4 needs --data scenes"),
                            (val, ["--data", "dataset", "--tta", "hflip"], "--tta hflip needs --data scenes"),
                            (val, ["--data", "tiles.npz", "--tta", "flips"], "--data tiles.npz is not"),
                            (val, ["--data", "scenes", "--tta", "flips", "--multi_scales"], "cannot be combined with --multi_scales")):
        with pytest.raises(SystemExit) as e:
            mod.parse_args(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, (argv, text)


def test_val_passes_the_mode_to_the_evaluator(monkeypatch, tmp_path):
    from emrt_amd import val
    from emrt_amd.config import get_config
    fake_abi.install()
    try:
        write_scene_tree(str(tmp_path), [(64, 80)], sub=VAL_SUB)
        cfg = get_config()
        cfg.DATA.DATA_PATH = str(tmp_path)
        cfg.VAL.CROP_SIZE, cfg.VAL.STRIDE_SIZE = [64, 64], [48, 48]
        ev = val.scene_evaluator(_Model(6), cfg, "cpu", tta="d4", max_batch=16)
        assert ev.tta == "d4" and ev.codes == tuple(range(8)) and ev.max_batch == 16
        assert val.scene_evaluator(_Model(6), cfg, "cpu").tta == "none"
    finally:
        fake_abi.uninstall()
