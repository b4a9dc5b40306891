"""CPU: class-aware tile sampling for `train.py --data scenes` (DATA.SCENE_SAMPLING, include/emrt_hip_sampler.h) without a GPU.

  config    the new node, the new yaml, train.py's refusal of MODE "class" without --data scenes
  launches  MODE "uniform" issues today's launches and never loads the third library; MODE "class" puts one emrt_smp_class_redraw between the
            draw and the sample launch of both chains, with host arguments built once
  host      class probabilities and thresholds against the restatement (tests/class_sampler_reference.py) and by hand
  contract  the restatement's redraw over 20 000 samples: shares within 5 binomial standard deviations, windows around their anchors
  library   the third header parses, the library exports exactly its entry points and refuses bad arguments; the build table of three"""
import argparse
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from emrt_amd.config import get_config, update_config
from emrt_amd.src import datasets as D
from emrt_amd.src.datasets import SceneBank, SceneSampler, class_probabilities, class_thresholds, label_lut
from tests import class_sampler_reference as R
from tests.test_augment_ext_cpu import FakeAugLib, aug_chain
from tests.test_scene_sampler_cpu import potsdam_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RCS = os.path.join(ROOT, "emrt_amd/configs/EMRT/EMRT_256x256_160k_potsdam_rcs.yaml")
SIZES = [(40, 56), (33, 47), (64, 64)]
NCLS = 4
CLASS = {"MODE": "class", "PROB": 0.5, "TEMPERATURE": 0.1, "CLASS_PROBS": None}


# ---- configuration ------------------------------------------------------------------------------------------------------------------------------

def test_config_carries_the_sampling_node_and_the_yaml_loads():
    node = get_config().DATA.SCENE_SAMPLING
    assert dict(node) == {"MODE": "uniform", "PROB": 0.5, "TEMPERATURE": 0.1, "CLASS_PROBS": None}
    cfg = update_config(get_config(), argparse.Namespace(cfg=RCS))
    assert dict(cfg.DATA.SCENE_SAMPLING) == CLASS
    base = update_config(get_config(), argparse.Namespace(cfg=os.path.join(os.path.dirname(RCS), "EMRT_256x256_160k_potsdam.yaml")))
    assert base.DATA.SCENE_SAMPLING.MODE == "uniform"
    assert {k: v for k, v in cfg.DATA.items() if k != "SCENE_SAMPLING"} == {k: v for k, v in base.DATA.items() if k != "SCENE_SAMPLING"}
    assert cfg.MODEL == base.MODEL and cfg.TRAIN == base.TRAIN


@pytest.mark.parametrize("data", ["synthetic", "dataset"])
def test_train_refuses_class_mode_without_resident_scenes(data):
    from emrt_amd import train
    with pytest.raises(SystemExit, match="SCENE_SAMPLING.MODE 'class' needs --data scenes .*--data %s has none" % data):
        train.main(["--config", RCS, "--data", data, "--no-eval", "--iters", "1"])


# ---- launches through the recording ABIs --------------------------------------------------------------------------------------------------------

class FakeSmpLib:
    """Recording stand-in for libemrt_hip_sampler.so: checks argument count and kinds against include/emrt_hip_sampler.h and logs.  The one thing it
    computes is the count table of emrt_smp_row_counts, with np.bincount from the label maps it was given (the bank lives in host memory here)."""

    def __init__(self, labels):
        from emrt_amd import _lib
        self.protos = _lib.parse_header(_lib.SMP_HEADER)
        self.labels, self.calls = labels, []

    def call(self, name, *args):
        spec = self.protos[name][1]
        assert len(args) == len(spec), "%s: %d args given, header declares %d" % (name, len(args), len(spec))
        for a, (t, an) in zip(args, spec):
            if t.endswith("*"):
                assert a is None or isinstance(a, (ctypes.c_void_p, int, ctypes.Array)), "%s.%s: bad pointer %r" % (name, an, a)
            elif t in ("float", "double"):
                assert isinstance(a, (int, float)) and not isinstance(a, bool), "%s.%s: expected a number, got %r" % (name, an, a)
            else:
                assert isinstance(a, int) and not isinstance(a, bool), "%s.%s (%s): expected int, got %r" % (name, an, t, a)
        self.calls.append((name, args))
        if name == "emrt_smp_row_counts":
            lut = None if args[7] is None else np.frombuffer(ctypes.string_at(args[7].value, 256), dtype=np.uint8)
            want = R.row_counts(self.labels, args[8], lut).astype(np.int32)
            assert args[10] == want.shape[0]
            ctypes.memmove(args[9].value, want.ctypes.data, want.nbytes)


@pytest.fixture
def bank_and_fakes(monkeypatch, tmp_path):
    from emrt_amd import _lib
    from tests import fake_abi
    labels = R.rare_class_labels(SIZES)
    root = str(tmp_path / "s")
    R.write_bank(root, SIZES, labels)
    main, aug, smp = fake_abi.install(), FakeAugLib(), FakeSmpLib(labels)
    monkeypatch.setattr(_lib, "_AUG_LIB", aug)
    monkeypatch.setattr(_lib, "_SMP_LIB", smp)
    yield SceneBank(root, "cpu"), labels, main, aug, smp
    fake_abi.uninstall()


def _buffers(B=8, hw=(32, 32)):
    return torch.empty(B, 3, *hw), torch.empty(B, *hw, dtype=torch.int64)


@pytest.mark.parametrize("sampling", [None, {"MODE": "uniform", "PROB": 0.5, "TEMPERATURE": 0.1, "CLASS_PROBS": None}, "config"])
def test_uniform_mode_issues_todays_launches_and_never_loads_the_third_library(bank_and_fakes, monkeypatch, sampling):
    from emrt_amd import _lib
    bank, _, main, aug, smp = bank_and_fakes
    monkeypatch.setattr(_lib, "_SMP_LIB", None)
    monkeypatch.setattr(_lib, "sampler_lib", lambda: (_ for _ in ()).throw(AssertionError("uniform sampling loaded the third library")))
    if sampling == "config":
        sampling = get_config().DATA.SCENE_SAMPLING
    images, labels = _buffers()
    s = SceneSampler(bank, potsdam_chain((32, 32)), 8, 1234, 3, sampling=sampling, num_classes=NCLS)
    assert not s.class_mode and s.class_table is None
    main.calls.clear()
    s.fill(images, labels)
    assert [n for n, _ in main.calls] == ["emrt_scene_draw", "emrt_scene_sample"] and aug.calls == [] and smp.calls == []
    e = SceneSampler(bank, aug_chain((32, 32), vflip=0.25, rng=0.3, prob=0.6), 8, 1234, 3, sampling=sampling, num_classes=NCLS)
    main.calls.clear()
    e.fill(images, labels)
    assert main.calls == [] and [n for n, _ in aug.calls] == ["emrt_aug_scene_draw", "emrt_aug_scene_sample"] and smp.calls == []
    assert _lib._SMP_LIB is None


@pytest.mark.parametrize("cols", [10, 18])
def test_class_mode_puts_one_redraw_between_draw_and_sample(bank_and_fakes, monkeypatch, cols):
    bank, labs, main, aug, smp = bank_and_fakes
    order = []
    for lib in (main, aug, smp):
        call = lib.call
        monkeypatch.setattr(lib, "call", lambda name, *a, _c=call: (order.append(name), _c(name, *a))[1])
    chain = potsdam_chain((32, 32)) if cols == 10 else aug_chain((32, 32), vflip=0.25, rng=0.3, prob=0.6)
    s = SceneSampler(bank, chain, 8, 1234, 3, sampling=dict(CLASS, PROB=0.25), num_classes=NCLS)
    assert order == ["emrt_smp_row_counts"] and s.class_mode and s.draws.shape == (8, cols)
    images, labels = _buffers()
    uploads = []
    real_to = torch.Tensor.to
    for _ in range(2):
        with monkeypatch.context() as m:          # a captured step can neither upload nor make tensors of host arrays
            m.setattr(torch.Tensor, "to", lambda self, *a, **k: (uploads.append(a), real_to(self, *a, **k))[1])
            m.setattr(torch, "from_numpy", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fill() made a host array into a tensor")))
            s.fill(images, labels)
    first, second = ("emrt_scene_draw", "emrt_scene_sample") if cols == 10 else ("emrt_aug_scene_draw", "emrt_aug_scene_sample")
    assert order[1:] == [first, "emrt_smp_class_redraw", second] * 2 and uploads == []
    a, b = smp.calls[1][1], smp.calls[2][1]
    from emrt_amd import runtime
    scenes_dev, _, scenes_host, _ = bank.tables(32, 32)
    idx = s.index
    assert a[0].value == runtime.ctx().step_counter.data_ptr() and a[1].value == bank.buffer.data_ptr() and a[2] == bank.nbytes
    assert a[3].value == scenes_dev.data_ptr() and a[4].value == ctypes.addressof(scenes_host)
    assert a[5].value == idx.row_start_dev.data_ptr() and a[6].value == ctypes.addressof(idx.row_start_host) and a[7] == 3
    assert a[8].value == idx.cum_dev.data_ptr() and a[9].value == s._thr_dev.data_ptr() and a[10].value == ctypes.addressof(s._thr_host)
    assert a[11:19] == (NCLS, None, 1234, 3, 8, 32, 32, 0.25) and a[19].value == s.draws.data_ptr() and a[20] == cols
    for i in (4, 6, 10, 12):          # the HOST arguments: the same objects in every call
        assert a[i] is b[i], i
    assert [type(x) for x in a] == [type(x) for x in b] and all(x == y for x, y in zip(a[11:19], b[11:19]))
    # what the constructor uploaded is the restatement's index
    counts = R.row_counts(labs, NCLS)
    assert np.array_equal(idx.counts, counts) and idx.totals.tolist() == counts.sum(0).tolist() and idx.totals[2] == 3 and idx.totals[3] == 0
    assert idx.cum.shape == (NCLS, sum(H for H, _ in SIZES) + 1) and np.array_equal(idx.cum[:, 1:], np.cumsum(counts.T, axis=1)) and not idx.cum[:, 0].any()
    assert idx.cum_dev.dtype == torch.int64 and np.array_equal(idx.cum_dev.numpy(), idx.cum)
    assert idx.row_start.tolist() == [0, 40, 73, 137] == list(idx.row_start_host) == idx.row_start_dev.tolist()
    assert [int(v) for v in s._thr_host] == R.thresholds(R.probabilities(counts.sum(0))) == s._thr_dev.tolist()
    assert [t[0] for t in s.class_table] == ["class %d" % c for c in range(NCLS)] and s.class_table[3][1:] == (0.0, 0.0)


def test_class_mode_goes_through_the_label_shift_and_says_what_is_absent(bank_and_fakes, tmp_path, capsys):
    """LoveDA's stored maps (classes one higher, 0 = ignore) through label_lut(1) index as the unshifted maps do; the absent class is named."""
    _, labs, main, aug, smp = bank_and_fakes
    shifted = R.rare_class_labels(SIZES, shift=1)
    root = str(tmp_path / "loveda")
    R.write_bank(root, SIZES, shifted)
    smp.labels = shifted
    from emrt_amd.src import transforms as T
    s = SceneSampler(SceneBank(root, "cpu", label_shift=1), [T.Normalize(mean=T._MEAN, std=T._STD)], 4, 1, 0, tile=(32, 32), sampling=CLASS,
                     num_classes=NCLS, class_names=["road", "roof", "car", "water"])
    assert np.array_equal(s.index.counts, R.row_counts(labs, NCLS)) and np.array_equal(s.index.counts, R.row_counts(shifted, NCLS, label_lut(1)))
    assert "water has no pixel in the bank: its sampling probability is 0" in capsys.readouterr().out
    s.fill(*_buffers(4))
    lut = ctypes.cast(smp.calls[-1][1][12], ctypes.POINTER(ctypes.c_ubyte))
    assert smp.calls[-1][0] == "emrt_smp_class_redraw" and [lut[i] for i in range(256)] == label_lut(1).tolist()


def test_class_mode_refusals(bank_and_fakes):
    bank = bank_and_fakes[0]
    mk = lambda **k: SceneSampler(bank, potsdam_chain((32, 32)), 8, 1, 0, **k)
    with pytest.raises(ValueError, match="MODE must be 'uniform' or 'class'"):
        mk(sampling=dict(CLASS, MODE="rare"), num_classes=NCLS)
    with pytest.raises(ValueError, match="needs num_classes"):
        mk(sampling=CLASS)
    with pytest.raises(ValueError, match=r"PROB 1.5 is outside \[0, 1\]"):
        mk(sampling=dict(CLASS, PROB=1.5), num_classes=NCLS)
    with pytest.raises(ValueError, match="CLASS_PROBS must be 4 finite non-negative weights"):
        mk(sampling=dict(CLASS, CLASS_PROBS=[1, 1, 1]), num_classes=NCLS)
    with pytest.raises(ValueError, match="TEMPERATURE must be finite and at least"):
        mk(sampling=dict(CLASS, TEMPERATURE=0.0), num_classes=NCLS)


# ---- probabilities and thresholds -----------------------------------------------------------------------------------------------------------------

def test_thresholds_follow_the_formula_on_a_hand_made_count_vector():
    totals = [700, 250, 50, 0, 0]                      # f = 0.7, 0.25, 0.05; two absent classes at the end
    p = class_probabilities(totals, 0.1)
    w = [math.exp(3.0), math.exp(7.5), math.exp(9.5)]
    assert np.allclose(p[:3], np.asarray(w) / sum(w), rtol=1e-12, atol=0) and p[3] == 0.0 and p[4] == 0.0 and abs(p.sum() - 1.0) < 1e-15
    thr = class_thresholds(p)
    assert thr.dtype == np.uint64 and thr.tolist() == R.thresholds(R.probabilities(totals, 0.1))
    assert thr[0] == math.floor(2.0 ** 32 * p[0]) and abs(int(thr[1]) - 2.0 ** 32 * (w[0] + w[1]) / sum(w)) <= 1.0
    assert thr.tolist()[2:] == [1 << 32] * 3           # the last class with pixels: exactly 2^32, and every class after it
    assert [R.pick_class(wd, thr.tolist()) for wd in (0, int(thr[0]) - 1, int(thr[0]), int(thr[1]) - 1, int(thr[1]), 0xFFFFFFFF)] == [0, 0, 1, 1, 2, 2]


def test_an_absent_class_gets_zero_and_leaves_its_neighbours_threshold_alone():
    p = class_probabilities([500, 0, 300, 200], 0.1)
    thr = class_thresholds(p).tolist()
    assert p[1] == 0.0 and thr[1] == thr[0] and thr[3] == 1 << 32 and thr == R.thresholds(R.probabilities([500, 0, 300, 200]))
    assert all(R.pick_class(wd, thr) != 1 for wd in (0, thr[0] - 1, thr[0], thr[0] + 1, thr[2], 0xFFFFFFFF))
    q = class_probabilities([500, 0, 300, 200], 0.1, class_probs=[1, 5, 1, 2])          # ... even under CLASS_PROBS
    assert q.tolist() == [0.25, 0.0, 0.25, 0.5] and class_thresholds(q).tolist() == [1 << 30, 1 << 30, 1 << 31, 1 << 32]
    z = class_thresholds(class_probabilities([5, 5, 5, 5], class_probs=[1, 3, 0, 0])).tolist()          # zero weights at the end
    assert z == [1 << 30, 1 << 32, 1 << 32, 1 << 32] and R.pick_class(0xFFFFFFFF, z) == 1


def test_a_bank_without_a_countable_pixel_is_refused():
    with pytest.raises(ValueError, match="holds no pixel of any of the 4 classes"):
        class_probabilities([0, 0, 0, 0])
    with pytest.raises(ValueError, match="gives no weight to a class that has pixels"):
        class_probabilities([0, 7, 0, 0], class_probs=[1, 0, 1, 1])


# ---- the contract, on the restatement -------------------------------------------------------------------------------------------------------------

def test_restatement_has_the_promised_distribution_and_windows():
    """20 steps of 1000 samples on the three-scene bank, 24 x 40 tile, PROB 0.5, the formula at T = 0.1.  Seeded: deterministic."""
    labels = R.rare_class_labels(SIZES)
    tile, prob = (24, 40), 0.5
    counts = R.row_counts(labels, NCLS)
    totals = counts.sum(0)
    assert totals[2] == 3 and totals[3] == 0
    p = R.probabilities(totals)
    thr = R.thresholds(p)
    base = [[0, 1, 2] + [7] * 7 for _ in range(1000)]
    rows, info = [], []
    for step in range(20):
        out, inf = R.redraw(base, 1234, step, 0, labels, tile, NCLS, thr, prob, counts=counts)
        rows += out
        info += inf
    n = len(rows)
    sig = lambda m, q: 5.0 * math.sqrt(m * q * (1.0 - q))
    hit = [i for i in info if i is not None]
    assert n == 20000 and abs(len(hit) - n * prob) <= sig(n, prob), len(hit)
    for r, i in zip(rows, info):          # a row is rewritten in columns 0-2 only, and only when its class decision fired
        assert r[3:] == [7] * 7 and (i is not None or r[:3] == [0, 1, 2])
    for c in range(NCLS):
        cnt = sum(i[0] == c for i in hit)
        assert abs(cnt - len(hit) * p[c]) <= sig(len(hit), p[c]), (c, cnt, len(hit) * p[c])
    assert not any(i[0] == 3 for i in hit)
    rare = [i for i in hit if i[0] == 2]
    anchors = [(0, 0, 0), (2, 63, 63), (2, 32, 32)]
    for a in anchors:
        cnt = sum(i[1:4] == a for i in rare)
        assert abs(cnt - len(rare) / 3) <= sig(len(rare), 1 / 3), (a, cnt, len(rare))
    assert sum(i[1:4] in anchors for i in rare) == len(rare)
    assert {i[4] for i in hit} == set(range(24)) and {i[5] for i in hit} == set(range(40))          # dy and dx reach 0 and th - 1 / tw - 1
    maps = R.mapped(labels)
    for r, i in zip(rows, info):
        if i is None:
            continue
        cls, s, y, x, dy, dx = i
        H, W = SIZES[s]
        s_, y0, x0 = r[:3]
        assert s_ == s and 0 <= y0 <= H - 24 and 0 <= x0 <= W - 40 and y0 <= y < y0 + 24 and x0 <= x < x0 + 40
        assert maps[s][y, x] == cls == maps[s][y0:y0 + 24, x0:x0 + 40][y - y0, x - x0]
        if 0 <= y - dy <= H - 24 and 0 <= x - dx <= W - 40:          # not clamped: the anchor sits at the drawn position
            assert (y - y0, x - x0) == (dy, dx)
    first = [r for r, i in zip(rows, info) if i is not None and i[1:4] == (0, 0, 0)]
    last = [r for r, i in zip(rows, info) if i is not None and i[1:4] == (2, 63, 63)]
    assert first and last and all(r[:3] == [0, 0, 0] for r in first) and all(r[:3] == [2, 64 - 24, 64 - 40] for r in last)


def test_restatement_leaves_rows_alone_when_the_index_is_stale():
    """Counts of another bank: whatever the redraw then does, a rewritten row is a window of its scene that holds a pixel of its class."""
    labels, other = R.rare_class_labels(SIZES), R.rare_class_labels(SIZES, seed=9)
    stale = R.row_counts(other, NCLS)
    thr = R.thresholds(R.probabilities(stale.sum(0)))
    base = [[1, 0, 0] + [7] * 7 for _ in range(2000)]
    rows, info = R.redraw(base, 99, 0, 0, labels, (24, 40), NCLS, thr, 1.0, counts=stale)
    assert any(i is None for i in info) and any(i is not None for i in info)
    maps = R.mapped(labels)
    for r, i in zip(rows, info):
        H, W = SIZES[r[0]]
        assert 0 <= r[1] <= H - 24 and 0 <= r[2] <= W - 40
        assert i is None or maps[i[1]][i[2], i[3]] == i[0]


# ---- the third library ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    from emrt_amd import build_ext
    build_ext.build(verbose=False)
    return build_ext


def test_third_library_exports_exactly_what_its_header_declares(built):
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.SMP_HEADER)
    assert sorted(protos) == ["emrt_smp_class_redraw", "emrt_smp_last_error", "emrt_smp_row_counts", "emrt_smp_version"]
    out = subprocess.run(["nm", "-D", "--defined-only", built.library("sampler").lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {n for n in exported if n.startswith("emrt_")} == set(protos)
    assert not set(protos) & (set(_lib.parse_header()) | set(_lib.parse_header(_lib.AUG_HEADER)))          # nothing is declared twice
    assert len(_lib.parse_header()) == 109 and len(_lib.parse_header(_lib.AUG_HEADER)) == 6                # the other two headers are untouched
    assert [len(a) for _, a in (protos["emrt_smp_row_counts"], protos["emrt_smp_class_redraw"])] == [12, 22]
    assert _lib.SMP_HEADER in built._headers() and os.path.join(built.CSRC, "philox.hpp") in built._headers()


def test_loader_of_the_third_library(built, monkeypatch, tmp_path):
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_SMP_LIB", None)
    S = _lib.sampler_lib()
    assert S.query("emrt_smp_version") == 1 and S is _lib.sampler_lib() and sorted(S.protos) == sorted(_lib.parse_header(_lib.SMP_HEADER))
    monkeypatch.setitem(_lib.SIDE_LIBRARIES, "sampler", _lib.SIDE_LIBRARIES["sampler"]._replace(path=str(tmp_path / "nope.so")))
    monkeypatch.setattr(_lib, "_SMP_LIB", None)
    with pytest.raises(_lib.EmrtHipError, match="not found"):
        _lib.sampler_lib()


def test_philox_is_written_once():
    """The generator and the integer draw live in csrc/philox.hpp; the three sources that draw include it and none restates it."""
    csrc = os.path.join(ROOT, "emrt_amd/csrc")
    assert "0xD2511F53" in open(os.path.join(csrc, "philox.hpp")).read()
    for f in ("augment.hip", "augment_ext/augment_ext.hip", "sampler_ext/sampler_ext.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert "philox.hpp\"" in text and "0xD2511F53" not in text and "__umul64hi" not in text, f


def test_build_rebuilds_only_the_third_library_when_its_source_changes(built):
    """Content stamps (tests/test_abi_cpu.py) with the third group: a touched source is "reused"; one more byte in it compiles that one object
    and links that one library, and the recorded digest follows.  The source is put back and rebuilt before the test ends."""
    src = os.path.join(built.library("sampler").dir, built.library("sampler").sources[0])
    assert os.path.dirname(src).endswith("sampler_ext")
    os.utime(src, None)
    built.build(verbose=False)
    assert built.LAST_BUILD["mode"] == "reused" and built.LAST_BUILD["compiled"] == [] and built.LAST_BUILD["linked"] == []
    before = built.source_digest()
    original = open(src, "rb").read()
    try:
        with open(src, "ab") as f:
            f.write(b"\n")
        assert built.source_digest() != before
        built.build(verbose=False)
        assert built.LAST_BUILD["compiled"] == ["sampler_ext.hip"] and built.LAST_BUILD["linked"] == ["libemrt_hip_sampler.so"]
        for row in built.LIBRARIES:
            with open(row.lib + ".inputs") as f:
                assert f.read().strip() == built.source_digest() == built.LAST_BUILD["digest"]
    finally:
        with open(src, "wb") as f:
            f.write(original)
        built.build(verbose=False)
    assert built.source_digest() == before and built.LAST_BUILD["compiled"] == ["sampler_ext.hip"]


def test_entry_points_refuse_bad_arguments_before_any_launch(built, monkeypatch):
    """Against the real library, no GPU: every bad call returns non-zero with a message before anything touches a device.  The device pointers
    are a made-up address and never dereferenced; the host mirrors are real arrays, and they are what is checked."""
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_SMP_LIB", None)
    S = _lib.sampler_lib()
    p = ctypes.c_void_p(0x10000)
    good = [(0, 3 * 40 * 56, 40, 56), (4 * 40 * 56, 4 * 40 * 56 + 3 * 64 * 64, 64, 64)]
    nbytes = 4 * 40 * 56 + 4 * 64 * 64
    entries = lambda rows: (D._SceneEntry * len(rows))(*[D._SceneEntry(*r) for r in rows])
    ll = lambda v: (ctypes.c_longlong * len(v))(*v)
    thr_ok = (1 << 30, 1 << 30, 1 << 31, 1 << 32)

    def counts(match, rows=good, starts=(0, 40, 104), bank=p, out=p, ncls=4, total=104, bank_bytes=nbytes):
        with pytest.raises(_lib.EmrtHipError, match=match):
            S.call("emrt_smp_row_counts", bank, bank_bytes, p, entries(rows), p, ll(starts), len(rows), None, ncls, out, total, None)

    def redraw(match, rows=good, starts=(0, 40, 104), thr=thr_ok, step=p, draws=p, cum=p, ncls=4, rank=0, B=8, th=32, tw=32, prob=0.5, cols=10,
               bank_bytes=nbytes):
        with pytest.raises(_lib.EmrtHipError, match=match):
            S.call("emrt_smp_class_redraw", step, p, bank_bytes, p, entries(rows), p, ll(starts), len(rows), cum, p,
                   (ctypes.c_ulonglong * len(thr))(*thr), ncls, None, 1234, rank, B, th, tw, prob, draws, cols, None)

    # (every case below must fail a check: one that passed would launch on the made-up pointers)
    counts("emrt_smp_row_counts: null pointer", bank=None)
    counts("null pointer", out=None)
    counts("n_classes must be 1..256", ncls=0)
    counts("n_classes must be 1..256", ncls=257)
    counts("n_scenes must be positive", rows=[], starts=(0,))
    counts("scene 1: image or label map outside the bank", bank_bytes=nbytes - 1)
    counts("scene 0: sizes must be positive", rows=[(0, 0, 0, 56)], starts=(0, 0))
    counts("scene 1: the row table holds 63 rows, the scene has 64", starts=(0, 40, 103), total=103)
    counts("row table must start at 0", starts=(1, 41, 105), total=105)
    counts("total_rows is not the last entry", total=105)
    redraw("emrt_smp_class_redraw: null pointer", step=None)
    redraw("null pointer", draws=None)
    redraw("null pointer", cum=None)
    redraw("B must be positive", B=0)
    redraw("32-bit counter word", rank=1 << 30)
    redraw("n_classes must be 1..256", ncls=0)
    redraw("class-mode probability must be in \\[0, 1\\]", prob=1.01)
    redraw("class-mode probability", prob=float("nan"))
    redraw("draw_cols must be 10 .* or 18", cols=12)
    redraw("scene 0: the 41x32 tile is larger than the 40x56 scene", th=41)
    redraw("scene 1: the 32x65 tile is larger than the 64x64 scene", rows=[(0, 3 * 80 * 80, 80, 80), good[1]], starts=(0, 80, 144), tw=65, bank_bytes=1 << 20)
    redraw("scene 1: image or label map outside the bank", bank_bytes=nbytes - 1)
    redraw("the row table holds", starts=(0, 41, 105))
    redraw("non-decreasing and at most 2\\^32", thr=(1 << 31, 1 << 30, 1 << 31, 1 << 32))
    redraw("non-decreasing and at most 2\\^32", thr=(1, 2, 3, (1 << 32) + 1))
    redraw("last class threshold must be exactly 2\\^32", thr=(1, 2, 3, (1 << 32) - 1))
