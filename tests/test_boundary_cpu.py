"""CPU: boundary-aware scene evaluation without a GPU -- the host model tests/boundary_reference.py against the scipy erosion
formulation, the invariant that ties its counts to metrics.calculate_area, libemrt_hip_bnd.so against its header and its refusals (host code:
every one returns before anything touches a device), the open lists of libraries, the launches SceneEvaluator(boundary=r) adds on recording
stand-ins, and the two new flags of emrt_amd.val."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import boundary_reference as BR
from tests.test_augment_ext_cpu import FakeAugLib
from tests.test_scene_eval_cpu import MEAN, STD, _bank, _evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blocky(rng, H, W, edge, values):
    """a class map of edge x edge blocks, cut off at an odd position"""
    oy, ox = int(rng.randint(0, edge)) | 1, int(rng.randint(0, edge)) | 1
    cells = rng.choice(np.asarray(values), ((H + oy) // edge + 2, (W + ox) // edge + 2))
    return np.kron(cells, np.ones((edge, edge), dtype=cells.dtype))[oy:oy + H, ox:ox + W].astype(np.uint8)


def band_by_erosion(M, r, shape):
    """1 - the union over the values c of binary_erosion(M == c, element, border_value=1)"""
    S = BR.structure(r, shape)
    interior = np.zeros(M.shape, dtype=bool)
    for c in np.unique(M):
        interior |= ndimage.binary_erosion(M == c, structure=S, border_value=1)
    return ~interior


# ---- the host model -----------------------------------------------------------------------------------------------------------------------------

def test_half_widths_are_the_integer_disk_and_the_square():
    assert BR.half_widths(3, "disk") == [0, 2, 2, 3, 2, 2, 0] and BR.half_widths(3, "square") == [3] * 7
    assert BR.half_widths(1, "disk") == [0, 1, 0] and BR.half_widths(5, "disk") == [0, 3, 4, 4, 4, 5, 4, 4, 4, 3, 0]
    for r in range(1, 33):
        for dy, w in zip(range(-r, r + 1), BR.half_widths(r, "disk")):
            assert w * w + dy * dy <= r * r < (w + 1) * (w + 1) + dy * dy
    with pytest.raises(ValueError, match="shape must be one of disk, square"):
        BR.half_widths(3, "diamond")


@pytest.mark.parametrize("shape", ["disk", "square"])
@pytest.mark.parametrize("H,W,r,kind", [(5, 7, 8, "blocks"), (1, 9, 2, "blocks"), (9, 1, 3, "blocks"), (23, 31, 3, "blocks"), (40, 37, 1, "noise"),
                                        (33, 50, 6, "blocks"), (20, 20, 3, "one"), (64, 70, 32, "blocks"), (30, 41, 3, "ignore")])
def test_host_model_equals_the_per_class_erosion(H, W, r, kind, shape):
    rng = np.random.RandomState(H * 100 + W + r)
    if kind == "one":
        M = np.full((H, W), 4, dtype=np.uint8)
    elif kind == "noise":
        M = rng.randint(0, 3, (H, W)).astype(np.uint8)
    else:
        M = blocky(rng, H, W, 6 if r < 32 else 40, [0, 1, 2, 3])
    if kind == "ignore":          # an ignore byte is a value like any other: a lone one and a block of them
        M[7, 9] = 255
        M[15:24, 20:33] = 255
    got = BR.band(M, r, shape)
    assert got.dtype == bool and np.array_equal(got, band_by_erosion(M, r, shape))
    if kind == "one":
        assert not got.any()
    if kind == "ignore":
        assert got[7, 9] and got[7, 9 + r] and not got[19, 26] and got[15, 26]
    # the two-pass form the kernels compute, from the model's own runs
    run, w = BR.runs(M, r).astype(np.int64), BR.half_widths(r, shape)
    two = np.zeros((H, W), dtype=bool)
    for dy in range(-r, r + 1):
        if abs(dy) < H:
            here, there = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
            two[here] |= (M[there] != M[here]) | (run[there] < w[dy + r])
    assert np.array_equal(two, got)


def test_runs_of_a_row_by_hand():
    M = np.array([[1, 1, 1, 2, 2, 2, 2, 2, 3]], dtype=np.uint8)
    assert BR.runs(M, 3).tolist() == [[2, 1, 0, 0, 1, 2, 1, 0, 0]]
    assert BR.runs(M[:, :1], 5).tolist() == [[5]]          # nothing in the image differs: the cap
    assert BR.runs(np.zeros((2, 3), np.int32), 32).tolist() == [[32] * 3] * 2


@pytest.mark.parametrize("shape", ["disk", "square"])
@pytest.mark.parametrize("ignore", [255, 0])
def test_eroded_areas_plus_the_areas_over_the_labels_band_are_calculate_area(shape, ignore):
    from emrt_amd.src.utils import metrics
    rng = np.random.RandomState(11)
    ncls = 5
    label = blocky(rng, 61, 83, 12, [0, 1, 2, 3, 4, 5, 255])          # 5 is outside the classes
    pred = blocky(rng, 61, 83, 12, [0, 1, 2, 3, 4, 5]).astype(np.int32)
    pred[rng.rand(61, 83) < 0.02] = -1
    agree = rng.rand(61, 83) < 0.5
    pred[agree] = label[agree]
    got = BR.counts(pred, label, ncls, ignore, 3, shape)
    assert got.shape == (2, 3, ncls) and got.dtype == np.int64
    bl = BR.band(label, 3, shape)
    on_band = BR.areas(pred, label, ncls, ignore, (bl, bl, bl))
    whole = torch.stack(metrics.calculate_area(torch.from_numpy(pred), torch.from_numpy(label), ncls, ignore)).numpy()
    assert np.array_equal(got[0] + on_band, whole) and got[0].sum() > 0 and on_band.sum() > 0
    # Boundary IoU's areas: the label row is the label area on the band; the intersection is inside both other rows
    assert np.array_equal(got[1][2], on_band[2]) and (got[1][0] <= got[1][1]).all() and (got[1][0] <= got[1][2]).all() and got[1][0].sum() > 0
    # a perfect prediction has Boundary IoU 1 wherever the class has a boundary
    clean = np.where(label < ncls, label, 0).astype(np.uint8)
    same = BR.counts(clean.astype(np.int32), clean, ncls, 255, 3, shape)
    assert np.array_equal(same[1][0], same[1][1]) and np.array_equal(same[1][0], same[1][2]) and np.array_equal(same[0][0], same[0][2])


# ---- the library --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    from emrt_amd import build_ext
    build_ext.build(verbose=False)
    return build_ext.library("bnd").lib


ENTRY_POINTS = ["emrt_bnd_areas", "emrt_bnd_band", "emrt_bnd_last_error", "emrt_bnd_runs", "emrt_bnd_version"]


def test_bnd_library_exports_exactly_what_its_header_declares(built):
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.BND_HEADER)
    assert sorted(protos) == ENTRY_POINTS
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in protos if n not in exported]
    assert not [n for n in exported if n.startswith("emrt_") and n not in protos]
    pinned = [_lib.parse_header()] + [_lib.parse_header(row.header) for row in _lib.SIDE_LIBRARIES.values()]
    rot = _lib.parse_header(_lib.ROT_HEADER)
    assert len(pinned) == 6 and not any(set(protos) & set(p) for p in pinned + [rot])          # nothing is declared twice
    assert [len(p) for p in pinned] == [109, 6, 4, 7, 4, 4] and len(rot) == 4                   # the seven headers before it are untouched
    assert _lib.parse_structs(_lib.BND_HEADER) == {}


def test_bnd_header_matches_its_definitions():
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.BND_HEADER)
    defs = {}
    for f in glob.glob(os.path.join(ROOT, "emrt_amd/csrc/bnd_ext/*.hip")):
        for m in re.finditer(r'extern "C" ([^{;]+?)\{', open(f).read(), re.S):
            p = re.sub(r"/\*.*?\*/", "", " ".join(m.group(1).split()))
            name = re.search(r"(\w+)\s*\(", p).group(1)
            args = p[p.index("(") + 1:p.rindex(")")]
            defs[name] = [] if args.strip() in ("", "void") else [re.match(r"(.*?)(\w+)$", " ".join(a.split())).group(1).strip() for a in args.split(",")]
    assert set(defs) == set(protos)
    for name, (ret, args) in protos.items():
        assert [t for t, _ in args] == defs[name], name
    text = open(_lib.BND_HEADER).read()
    assert "#define EMRT_BND_MAX_RADIUS %d\n" % BR.MAX_RADIUS in text
    assert all("#define EMRT_BND_%s %d\n" % (k.upper(), v) in text for k, v in BR.SHAPES.items())


def test_the_open_list_of_libraries(built):
    """build_ext.OPEN_LIBRARIES / _lib.OPEN_SIDE_LIBRARIES continue the two pinned tables: the bnd row is IN them (they may hold more) and is built,
    hashed, looked up and loaded like every other row."""
    from emrt_amd import _lib, build_ext
    assert "libemrt_hip_bnd.so" in [os.path.basename(r.lib) for r in build_ext.OPEN_LIBRARIES] and "bnd" in _lib.OPEN_SIDE_LIBRARIES
    assert [r.name for r in build_ext.OPEN_LIBRARIES] == list(_lib.OPEN_SIDE_LIBRARIES)
    assert build_ext.all_libraries() == build_ext.LIBRARIES + build_ext.LATER_LIBRARIES + build_ext.OPEN_LIBRARIES
    names = [r.name for r in build_ext.all_libraries()]
    assert len(set(names)) == len(names) and names[1:] == list(_lib.side_libraries())
    slots = [s.slot for s in _lib.side_libraries().values()]
    assert len(set(slots)) == len(slots) and all(hasattr(_lib, s) for s in slots)
    digest = build_ext.source_digest()
    for row in build_ext.OPEN_LIBRARIES:
        assert type(row) is build_ext.Library and build_ext.library(row.name) is row and row.header in build_ext._headers()
        assert all(os.path.exists(os.path.join(row.dir, s)) for s in row.sources)
        side = _lib.OPEN_SIDE_LIBRARIES[row.name]
        assert type(side) is _lib.SideLibrary and (side.header, side.path) == (row.header, os.environ.get(side.env) or row.lib)
    row, side = build_ext.library("bnd"), _lib.OPEN_SIDE_LIBRARIES["bnd"]
    assert row.sources == ["bnd_ext.hip"] and row.dir.endswith(os.path.join("csrc", "bnd_ext")) and os.path.basename(row.header) == "emrt_hip_bnd.h"
    assert (side.slot, side.prefix, side.env) == ("_BND_LIB", "emrt_bnd", "EMRT_HIP_BND_LIB")
    for r in build_ext.all_libraries():          # every library's stamp is the one digest of them all
        with open(r.lib + ".inputs") as f:
            assert os.path.exists(r.lib) and f.read().strip() == digest
    with pytest.raises(KeyError, match="no library 'nope'"):
        build_ext.library("nope")


def test_the_digest_covers_the_bnd_source_and_header(built):
    from emrt_amd import build_ext
    row = build_ext.library("bnd")
    inputs = [os.path.join(r.dir, s) for r in build_ext.all_libraries() for s in r.sources] + build_ext._headers()
    assert os.path.join(row.dir, "bnd_ext.hip") in inputs and row.header in inputs
    assert build_ext.source_digest() == build_ext._digest(inputs, [build_ext._hipcc()] + build_ext.FLAGS)
    without = [p for p in inputs if p != row.header]
    assert build_ext._digest(without, [build_ext._hipcc()] + build_ext.FLAGS) != build_ext.source_digest()


def test_loader_of_the_bnd_library(built, monkeypatch, tmp_path):
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_BND_LIB", None)
    B = _lib.bnd_lib()
    assert B.query("emrt_bnd_version") == 1 and B is _lib.bnd_lib() and B is _lib.side_lib("bnd") and sorted(B.protos) == ENTRY_POINTS
    monkeypatch.setitem(_lib.OPEN_SIDE_LIBRARIES, "bnd", _lib.OPEN_SIDE_LIBRARIES["bnd"]._replace(path=str(tmp_path / "nope.so")))
    monkeypatch.setattr(_lib, "_BND_LIB", None)
    with pytest.raises(_lib.EmrtHipError, match=r"nope\.so not found.*no CPU/PyTorch fallback for the boundary-aware scene evaluation"):
        _lib.bnd_lib()
    assert _lib.side_lib("rot") is _lib.rot_lib()          # the rows of the other lists are found as before


def test_entry_points_refuse_bad_arguments_before_any_launch(built, monkeypatch):
    """Against the real library, no GPU: every bad call returns non-zero with a message naming the argument before anything touches a device.
    The device pointers are a made-up address, never dereferenced."""
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_BND_LIB", None)
    B = _lib.bnd_lib()
    p = ctypes.c_void_p(0x10000)

    def refused(match, name, *args):
        with pytest.raises(_lib.EmrtHipError, match=match) as e:
            B.call(name, *args)
        assert "launch failed" not in str(e.value) and str(e.value).startswith(name + " failed")
        assert re.search(match, B.last_error())

    for name, args in (("emrt_bnd_runs", lambda m=p, kind=0, H=8, W=8, r=3, out=p: (m, kind, H, W, r, out, None)),
                       ("emrt_bnd_band", lambda m=p, kind=0, H=8, W=8, r=3, out=p, runs=p, shape=0: (m, kind, runs, H, W, r, shape, out, None))):
        refused(name + ": null pointer", name, *args(m=None))
        refused(name + ": null pointer", name, *args(out=None))
        for kind in (1, 3, -1):          # 1 is int64 in emrt_segmentation_areas: no map of this library
            refused(name + ": map_kind selects the map's type: 0 = int32, 2 = uint8", name, *args(kind=kind))
        for r in (0, 33, -3):
            refused(name + r": radius must be 1\.\.32", name, *args(r=r))
        for bad in (0, -5, 65537):
            refused(name + r": H must be 1\.\.65536", name, *args(H=bad))
            refused(name + r": W must be 1\.\.65536", name, *args(W=bad))
    refused("emrt_bnd_band: null pointer", "emrt_bnd_band", p, 2, None, 8, 8, 3, 0, p, None)
    for shape in (2, -1):
        refused(r"emrt_bnd_band: shape must be 0 \(disk\) or 1 \(square\)", "emrt_bnd_band", p, 2, p, 8, 8, 3, shape, p, None)
    for k in range(4):
        a = [p, p, p, p, 64, 6, 255, p, None]
        a[k] = None
        refused("emrt_bnd_areas: null pointer", "emrt_bnd_areas", *a)
    refused("emrt_bnd_areas: null pointer", "emrt_bnd_areas", p, p, p, p, 64, 6, 255, None, None)
    for ncls in (0, 257, -1):
        refused(r"emrt_bnd_areas: num_classes must be 1\.\.256", "emrt_bnd_areas", p, p, p, p, 64, ncls, 255, p, None)
    refused("emrt_bnd_areas: n must not be negative", "emrt_bnd_areas", p, p, p, p, -1, 6, 255, p, None)
    assert B.query("emrt_bnd_areas", p, p, p, p, 0, 256, 255, p, None) == 0          # nothing to count: nothing is launched


# ---- SceneEvaluator on recording stand-ins -------------------------------------------------------------------------------------------------------

class FakeBndLib(FakeAugLib):
    """Recording stand-in for libemrt_hip_bnd.so: checks argument count and kinds against include/emrt_hip_bnd.h, logs, computes nothing."""

    def __init__(self, log):
        from emrt_amd import _lib
        self.protos = _lib.parse_header(_lib.BND_HEADER)
        self.calls = log


@pytest.fixture
def fakes(monkeypatch):
    """the main library's stand-in and the boundary library's, logging into ONE list (the order across both is what is asserted)"""
    from emrt_amd import _lib
    from tests import fake_abi
    main = fake_abi.install()
    bnd = FakeBndLib(main.calls)
    monkeypatch.setattr(_lib, "_BND_LIB", bnd)
    yield main, bnd
    fake_abi.uninstall()


@pytest.mark.parametrize("shape,code", [("disk", 0), ("square", 1)])
def test_boundary_adds_five_launches_after_each_scenes_areas(fakes, tmp_path, shape, code):
    main, _ = fakes
    sizes = [(64, 80), (70, 64), (64, 80)]
    bank, _ = _bank(tmp_path, sizes)
    _, ev = _evaluator(bank, boundary=3, boundary_shape=shape, ignore_index=250)
    assert main.calls == [] and ev.boundary == 3 and ev.boundary_shape == code
    assert ev.boundary_per_scene.shape == (3, 2, 3, 6) and ev.boundary_per_scene.dtype == torch.int64
    tot = ev.evaluate()
    assert tot.shape == (3, 6) and ev.per_scene.shape == (3, 3, 6) and ev.boundary_totals().shape == (2, 3, 6)
    # both results are zeroed before the first scene
    first_scene = [n for n, _ in main.calls].index("emrt_scene_crop_windows_u8")
    zeroed = [a[0].value for n, a in main.calls[:first_scene] if n == "emrt_memset"]
    sizes_zeroed = [a[2] for n, a in main.calls[:first_scene] if n == "emrt_memset"]
    assert zeroed[:2] == [ev.per_scene.data_ptr(), ev.boundary_per_scene.data_ptr()] and sizes_zeroed[:2] == [3 * 3 * 6 * 8, 3 * 2 * 3 * 6 * 8]
    tail = [(n, a) for n, a in main.calls if n in ("emrt_argmax_nchw", "emrt_segmentation_areas") or n.startswith("emrt_bnd_")]
    assert len(tail) == 7 * 3
    base, scratch = bank.buffer.data_ptr(), []
    for i, (H, W) in enumerate(sizes):
        names = [n for n, _ in tail[7 * i:7 * i + 7]]
        assert names == ["emrt_argmax_nchw", "emrt_segmentation_areas", "emrt_bnd_runs", "emrt_bnd_band", "emrt_bnd_runs", "emrt_bnd_band", "emrt_bnd_areas"]
        arg, seg, run_p, band_p, run_l, band_l, areas = [a for _, a in tail[7 * i:7 * i + 7]]
        pred, label = arg[1].value, base + bank.offsets[i][1]
        assert seg[0].value == pred and seg[1].value == label
        assert (run_p[0].value, run_p[1:5]) == (pred, (0, H, W, 3)) and (run_l[0].value, run_l[1:5]) == (label, (2, H, W, 3))
        runs = run_p[5].value
        assert run_l[5].value == runs                                              # one runs map, used twice in stream order
        assert (band_p[0].value, band_p[1], band_p[2].value, band_p[3:7]) == (pred, 0, runs, (H, W, 3, code))
        assert (band_l[0].value, band_l[1], band_l[2].value, band_l[3:7]) == (label, 2, runs, (H, W, 3, code))
        bp, bl = band_p[7].value, band_l[7].value
        assert len({runs, bp, bl}) == 3
        assert [a.value for a in areas[:4]] == [pred, label, bp, bl] and areas[4:7] == (H * W, 6, 250)
        assert areas[7].value == ev.boundary_per_scene[i].data_ptr()
        stream = lambda a: getattr(a[-1], "value", a[-1])
        assert all(stream(a) == stream(seg) for a in (run_p, band_p, run_l, band_l, areas))          # the stream of the other launches
        scratch.append((runs, bp, bl))
    # scratch per scene shape: scenes 0 and 2 share theirs, and a second evaluation allocates nothing
    assert scratch[0] == scratch[2] and not set(scratch[0]) & set(scratch[1]) and len(ev._bnd_scratch) == 2 and len(ev._scratch) == 2
    del main.calls[:]
    ev.evaluate(rank=1, nranks=2)
    again = [a for n, a in main.calls if n == "emrt_bnd_areas"]
    assert len(again) == 1 and again[0][7].value == ev.boundary_per_scene[1].data_ptr() and (again[0][2].value, again[0][3].value) == scratch[1][1:]
    assert ev.boundary_per_scene.data_ptr() in [a[0].value for n, a in main.calls if n == "emrt_memset"]


def test_without_boundary_the_launches_are_todays_and_the_library_is_never_loaded(fakes, tmp_path, monkeypatch):
    from emrt_amd import _lib
    main, _ = fakes
    monkeypatch.setattr(_lib, "_BND_LIB", None)
    boom = lambda *a: (_ for _ in ()).throw(AssertionError("an evaluation without boundary= loaded libemrt_hip_bnd.so"))
    monkeypatch.setattr(_lib, "bnd_lib", boom)
    monkeypatch.setattr(_lib, "_ExtLib", boom)
    bank, _ = _bank(tmp_path, [(64, 80), (70, 64)])
    _, ev = _evaluator(bank)
    _, ev_none = _evaluator(bank, boundary=None, boundary_shape="square")
    ev.evaluate()
    plain = [(n, [type(a) for a in args]) for n, args in main.calls]
    del main.calls[:]
    ev_none.evaluate()
    assert [(n, [type(a) for a in args]) for n, args in main.calls] == plain
    names = [n for n, _ in main.calls if n != "emrt_memset"]
    assert names == ["emrt_scene_crop_windows_u8", "emrt_window_accumulate", "emrt_window_normalise", "emrt_argmax_nchw", "emrt_segmentation_areas"] * 2
    assert [n for n, _ in main.calls].count("emrt_memset") == 1 + 2 * 2          # per_scene, then sums and counts of each scene
    assert ev.boundary is None and ev.boundary_per_scene is None and ev._bnd_scratch == {} and _lib._BND_LIB is None
    with pytest.raises(ValueError, match="made without boundary="):
        ev.boundary_totals()


def test_boundary_refusals_before_anything_is_loaded(fakes, tmp_path, monkeypatch):
    from emrt_amd import _lib
    main, _ = fakes
    monkeypatch.setattr(_lib, "bnd_lib", lambda *a: (_ for _ in ()).throw(AssertionError("a refused evaluator loaded libemrt_hip_bnd.so")))
    bank, _ = _bank(tmp_path, [(64, 64)])
    for r in (0, 33, -1):
        with pytest.raises(ValueError, match=r"boundary must be a radius in 1\.\.32, got %d" % r):
            _evaluator(bank, boundary=r)
    for r in (3.0, "3", True, 2.5):
        with pytest.raises(ValueError, match="boundary must be an integer radius"):
            _evaluator(bank, boundary=r)
    for kw in ({"boundary": 3}, {}):
        with pytest.raises(ValueError, match="boundary_shape must be one of disk, square, got 'diamond'"):
            _evaluator(bank, boundary_shape="diamond", **kw)
    assert _evaluator(bank, boundary=np.int64(32))[1].boundary == 32 and _evaluator(bank, boundary=1)[1].boundary == 1
    assert main.calls == []


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------

def test_val_parses_boundary_with_scenes_only(capsys):
    from emrt_amd import val
    a = val.parse_args(["--data", "scenes", "--boundary", "3"])
    assert (a.boundary, a.boundary_shape) == (3, "disk")
    a = val.parse_args(["--data", "scenes", "--boundary", "32", "--boundary_shape", "square", "--tta", "d4", "--tta_scales", "0.75", "1.0"])
    assert (a.boundary, a.boundary_shape, a.tta, a.tta_scales) == (32, "square", "d4", [0.75, 1.0])
    a = val.parse_args(["--data", "scenes", "--multi_scales", "--boundary", "1"])
    assert a.boundary == 1 and a.multi_scales
    a = val.parse_args(["--data", "scenes"])
    assert (a.boundary, a.boundary_shape) == (None, "disk")
    for argv, message in ((["--boundary", "3"], "--boundary needs --data scenes"),
                          (["--data", "dataset", "--boundary", "3"], "--boundary needs --data scenes"),
                          (["--data", "x.npz", "--boundary", "3"], "--boundary needs --data scenes"),
                          (["--data", "scenes", "--boundary", "0"], r"boundary must be a radius in 1\.\.32"),
                          (["--data", "scenes", "--boundary", "33"], r"boundary must be a radius in 1\.\.32"),
                          (["--data", "scenes", "--boundary", "2.5"], "invalid int value"),
                          (["--data", "scenes", "--boundary", "3", "--boundary_shape", "diamond"], "invalid choice"),
                          (["--data", "scenes", "--boundary_shape", "square"], "--boundary_shape needs --boundary")):
        with pytest.raises(SystemExit) as e:
            val.parse_args(argv)
        assert e.value.code == 2 and re.search(message, capsys.readouterr().err), argv


def test_boundary_lines_print_the_metrics_of_the_totals():
    from types import SimpleNamespace
    from emrt_amd import val
    from emrt_amd.src.utils import metrics
    tot = torch.tensor([[[50, 30, 0], [60, 40, 5], [55, 45, 0]], [[8, 3, 0], [10, 9, 2], [16, 4, 0]]], dtype=torch.int64)
    ev = SimpleNamespace(boundary=3, boundary_shape=1, boundary_totals=lambda: tot.clone())
    lines = val.boundary_lines(ev)
    miou, acc, _, _, _, cf1, mf1 = val.metric_tuple(tot[0])
    biou, mbiou = metrics.mean_iou(tot[1][0], tot[1][1], tot[1][2])
    assert lines == ["[EVAL] Eroded (square r=3): mIoU: %.4f  Acc: %.4f  mF1: %.4f" % (miou, acc, mf1), "[EVAL] Eroded Class F1-score: " + str(np.round(cf1, 4)),
                     "[EVAL] Boundary (square r=3): mBIoU: %.4f" % mbiou, "[EVAL] Boundary Class BIoU: " + str(np.round(biou, 4))]
    assert np.allclose(biou, [8 / 18, 3 / 10, 0.0]) and abs(acc - 80 / 105) < 1e-12
