"""CPU: the quarter turn of the training augmentation (RandomRot90, DATA.AUGMENT.ROT90_PROB) through every host layer, without a GPU.

  transform     RandomRot90 equals np.rot90 on image and label for every k; prob 0 and 1; the draws it consumes
  config        the default chains are today's; the key's position with / without vertical flip and distortion; LoveDA and a non-square crop
                are refused by name; the d4 yaml; ROTATE_PROB stays unknown
  DevicePlan    the four new chains, the same decisions and generator state as the CPU chain, RotPlan around the old tuples
  draws         the Philox block-5 draw restated in Python (rot_turns; tests/test_gpu_rot90.py holds the kernel to it): distribution; the
                composite with the flips is uniform on D4; the turns are the variant codes 0, 5, 3, 6 of --tta d4
  library       libemrt_hip_rot.so exports what include/emrt_hip_rot.h declares, the loader, the host-side refusals, the second list of
                libraries, and that the default key never asks for the library"""
import argparse
import ctypes
import glob
import itertools
import math
import os
import random
import re
import subprocess
import threading

import numpy as np
import pytest
import torch

from emrt_amd.config import get_config, update_config
from emrt_amd.src import datasets as D
from emrt_amd.src import transforms as T
from emrt_amd.src.datasets import SceneBank, SceneSampler
from tests.test_augment_ext_cpu import FakeAugLib, _cfg, _forced, _params, _same_state, _seed, _states, _tile_tree, aug_chain
from tests.test_scene_sampler_cpu import M32, below, philox4x32_10, potsdam_chain, write_scene_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "emrt_amd/configs/EMRT")
ROT_BLOCK = 5                # include/emrt_hip_rot.h: EMRT_ROT_BLOCK
KEY = 1234                   # the key of the other sampler tests; the distribution check below passes with it (the counts are in its docstring)
TURN_CODES = (0, 5, 3, 6)    # turn k as a variant code of include/emrt_hip_tta.h (t * 4 + fv * 2 + fh)


def rot_chain(crop_wh, vflip=0.5, distort=True, rot=0.75, **kw):
    """aug_chain with RandomRot90 at its position: after the flips, before RandomDistort and Normalize."""
    chain = aug_chain(crop_wh, vflip=vflip, distort=distort, **kw)
    at = 3 + (vflip is not None)
    return chain[:at] + [T.RandomRot90(prob=rot)] + chain[at:]


def rot_turns(key, step, rank, B, prob):
    """The turns of emrt_rot_scene_batch, restated: Philox block 5 of the sample's counter; word 0 decides, words 1-2 pick k = 1 + below(3)."""
    k = (key & M32, (key >> 32) & M32)
    out = []
    for b in range(B):
        r = philox4x32_10([step & M32, (step >> 32) & M32, (rank * B + b) & M32, ROT_BLOCK], k)
        out.append(1 + below(r[1], r[2], 3) if r[0] * 2.0 ** -32 < prob else 0)
    return out


def variant(a, code):
    """Variant `code` of a window as include/emrt_hip_tta.h defines it: rows reversed if fv, columns reversed if fh, then transposed if t."""
    if code & 2:
        a = a[::-1]
    if code & 1:
        a = a[:, ::-1]
    return a.T if code & 4 else a


# ---- the transform ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_rot90_equals_numpy_for_every_turn(n):
    g = np.random.RandomState(n)
    img, lab = g.rand(n, n, 3).astype(np.float32), g.randint(0, 256, (n, n)).astype(np.uint8)
    t = T.RandomRot90(prob=1.0)
    for k in range(4):
        t.draw = lambda k=k: k
        gi, gl = t(img, lab)
        assert np.array_equal(gi, np.rot90(img, k, axes=(0, 1))) and np.array_equal(gl, np.rot90(lab, k, axes=(0, 1))), k
        assert len(t(img)) == 1 and np.array_equal(t(img)[0], np.rot90(img, k, axes=(0, 1)))
    if n > 1:          # counter-clockwise in array coordinates: the top right corner goes to the top left
        t.draw = lambda: 1
        assert t(img, lab)[1][0, 0] == lab[0, n - 1]


def test_rot90_probabilities_and_the_draws_it_consumes():
    img, lab = np.arange(48, dtype=np.float32).reshape(4, 4, 3), np.arange(16, dtype=np.uint8).reshape(4, 4)
    never, always = T.RandomRot90(prob=0.0), T.RandomRot90(prob=1.0)
    seen = set()
    for seed in range(60):
        random.seed(seed)
        assert never.draw() == 0
        random.seed(seed)
        random.random()
        after_one = random.getstate()                                         # prob 0: exactly one random.random()
        random.seed(seed)
        never(img, lab)
        assert random.getstate() == after_one
        random.seed(seed)
        random.random()
        want = 1 + random.randrange(3)
        after_two = random.getstate()
        random.seed(seed)
        k = always.draw()
        assert k == want and 1 <= k <= 3 and random.getstate() == after_two          # prob 1: random.random(), then random.randrange(3)
        random.seed(seed)
        gi, gl = always(img, lab)
        assert random.getstate() == after_two and np.array_equal(gi, np.rot90(img, k)) and np.array_equal(gl, np.rot90(lab, k))
        seen.add(k)
    assert seen == {1, 2, 3}
    # a seeded sequence at 0.75: per call one random.random() and, only where it passes, one random.randrange(3); np.random is never touched
    t = T.RandomRot90(prob=0.75)
    random.seed(7)
    np.random.seed(7)
    np_before = np.random.get_state()
    got = [t.draw() for _ in range(200)]
    after = random.getstate()
    random.seed(7)
    want = []
    for _ in range(200):
        want.append(1 + random.randrange(3) if random.random() < 0.75 else 0)
    assert got == want and random.getstate() == after and set(got) == {0, 1, 2, 3}
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(np_before, np.random.get_state()))
    with pytest.raises(ValueError, match="square"):
        always(np.zeros((4, 5, 3), np.float32))


# ---- chain and config ---------------------------------------------------------------------------------------------------------------------------

def test_the_default_key_leaves_the_chains_as_they_were():
    assert get_config().DATA.AUGMENT.ROT90_PROB == 0.0
    for name in ("EMRT_256x256_160k_potsdam.yaml", "EMRT_256x256_120k_vaihingen.yaml"):
        assert [_params(t) for t in T.get_transforms(_cfg(name))] == [_params(t) for t in potsdam_chain((256, 256))]
    assert [_params(t) for t in T.get_transforms(_cfg("EMRT_256x256_160k_loveda.yaml"))] == [_params(T.Normalize(mean=T._MEAN, std=T._STD))]
    assert [_params(t) for t in T.get_transforms(_cfg("EMRT_256x256_160k_potsdam_augment.yaml"))] == [_params(t) for t in aug_chain((256, 256))]
    cfg = _cfg()
    cfg.DATA.CROP_SIZE = (96, 64)          # a non-square crop is no concern of a chain without the key
    assert [type(t).__name__ for t in T.get_transforms(cfg)] == ["ResizeStepScaling", "RandomPaddingCrop", "RandomHorizontalFlip", "Normalize"]


@pytest.mark.parametrize("vflip,distort", [(False, False), (True, False), (False, True), (True, True)])
def test_the_key_inserts_the_op_at_the_stated_position(vflip, distort):
    cfg = _cfg()
    cfg.DATA.AUGMENT.ROT90_PROB = 0.6
    cfg.DATA.AUGMENT.VFLIP_PROB = 0.25 if vflip else 0.0
    cfg.DATA.AUGMENT.DISTORT.ENABLE = distort
    chain = T.get_transforms(cfg)
    want = (["ResizeStepScaling", "RandomPaddingCrop", "RandomHorizontalFlip"] + ["RandomVerticalFlip"] * vflip + ["RandomRot90"]
            + ["RandomDistort"] * distort + ["Normalize"])
    assert [type(t).__name__ for t in chain] == want
    assert chain[3 + vflip].prob == 0.6
    # ... and nothing else about the chain changes
    cfg.DATA.AUGMENT.ROT90_PROB = 0.0
    assert [_params(t) for t in T.get_transforms(cfg)] == [_params(t) for t in chain[:3 + vflip] + chain[4 + vflip:]]


def test_loveda_and_a_non_square_crop_are_refused_by_name():
    cfg = _cfg("EMRT_256x256_160k_loveda.yaml")
    cfg.DATA.AUGMENT.ROT90_PROB = 0.75
    with pytest.raises(ValueError, match=r"DATA\.AUGMENT\.ROT90_PROB.*LoveDA"):
        T.get_transforms(cfg)
    cfg = _cfg()
    cfg.DATA.AUGMENT.ROT90_PROB = 0.75
    cfg.DATA.CROP_SIZE = (96, 64)
    with pytest.raises(ValueError, match=r"DATA\.AUGMENT\.ROT90_PROB.*DATA\.CROP_SIZE.*\(96, 64\).*square"):
        T.get_transforms(cfg)
    with pytest.raises(ValueError, match="RandomRot90 needs a square crop, got 64x96"):
        T.DevicePlan(rot_chain((96, 64)))
    cfg.DATA.CROP_SIZE = (64, 64)
    cfg.DATA.AUGMENT.ROT90_PROB = 1.5
    with pytest.raises(ValueError, match=r"DATA\.AUGMENT\.ROT90_PROB must lie in \[0, 1\]"):
        T.get_transforms(cfg)


def test_train_refuses_a_non_square_crop_at_start_up(tmp_path):
    from emrt_amd import train
    bad = tmp_path / "bad.yaml"
    bad.write_text('BASE: ["%s"]\nDATA: {CROP_SIZE: "(96, 64)"}\n' % os.path.join(CFG_DIR, "EMRT_256x256_160k_potsdam_d4.yaml"))
    with pytest.raises(SystemExit, match=r"\[train\] DATA\.AUGMENT\.ROT90_PROB is set, but DATA\.CROP_SIZE is \(96, 64\)"):
        train.main(["--config", str(bad), "--data", "synthetic", "--no-eval", "--iters", "1"])


def test_the_d4_yaml_parses_and_rotate_prob_stays_unknown(tmp_path):
    cfg, aug = _cfg("EMRT_256x256_160k_potsdam_d4.yaml"), _cfg("EMRT_256x256_160k_potsdam_augment.yaml")
    assert cfg.DATA.DATASET == "Potsdam" and cfg.DATA.AUGMENT.ROT90_PROB == 0.75 and cfg.DATA.AUGMENT.VFLIP_PROB == 0.5
    assert {k: v for k, v in cfg.DATA.AUGMENT.items() if k != "ROT90_PROB"} == {k: v for k, v in aug.DATA.AUGMENT.items() if k != "ROT90_PROB"}
    assert cfg.MODEL == aug.MODEL and cfg.TRAIN == aug.TRAIN
    assert [_params(t) for t in T.get_transforms(cfg)] == [_params(t) for t in rot_chain((256, 256))]
    bad = tmp_path / "bad.yaml"
    bad.write_text("DATA: {AUGMENT: {ROTATE_PROB: 0.5}}\n")
    with pytest.raises(KeyError, match=r"DATA\.AUGMENT\.ROTATE_PROB"):
        update_config(get_config(), argparse.Namespace(cfg=str(bad)))


# ---- DevicePlan ---------------------------------------------------------------------------------------------------------------------------------

def _forced_rot(chain, p):
    """The chain with its draws replaced by the RotPlan's decisions (no RNG call)."""
    rot = next(t for t in chain if isinstance(t, T.RandomRot90))
    rest = [t for t in chain if t is not rot]
    base = p.base if isinstance(p.base, T.AugSamplePlan) else T.AugSamplePlan(*p.base, 0, ())
    _forced(rest, base)
    rot.draw = lambda: p.turn
    return T.Compose(chain)


@pytest.mark.parametrize("vflip,distort", [(None, False), (0.5, False), (None, True), (0.5, True)])
@pytest.mark.parametrize("src,crop", [((80, 96), (64, 64)), ((37, 41), (24, 24))])
def test_planner_draws_the_new_chains_decisions(vflip, distort, src, crop):
    """Per seed: the CPU chain, then (same seed) DevicePlan.plan: the same generator state afterwards, and the chain re-run with its draws forced
    to the plan's decisions gives the same arrays."""
    H, W = src
    g = np.random.RandomState(H * 1000 + W)
    img = g.randint(0, 256, (H, W, 3)).astype(np.float32)
    lab = g.randint(0, 6, (H, W)).astype(np.uint8)
    chain = lambda: rot_chain(crop, vflip=vflip, distort=distort)
    dp = T.DevicePlan(chain())
    assert dp.rot is not None and dp.rot.prob == 0.75 and dp.extended == (vflip is not None or distort)
    turns = set()
    for seed in range(40):
        _seed(seed)
        want_img, want_lab = T.Compose(chain())(img, lab)
        after = _states()
        _seed(seed)
        p = dp.plan(H, W)
        assert type(p) is T.RotPlan and p._fields == ("base", "turn") and _same_state(after, _states()), (seed, p)
        assert type(p.base) is (T.AugSamplePlan if dp.extended else T.SamplePlan) and p.turn in (0, 1, 2, 3)
        got_img, got_lab = _forced_rot(chain(), p)(img, lab)
        assert np.array_equal(want_img, got_img) and np.array_equal(want_lab, got_lab), (seed, p)
        turns.add(p.turn)
    assert turns == {0, 1, 2, 3} and dp.out_size(H, W) == (crop[1], crop[0])


def test_chains_without_the_op_keep_their_plans():
    for chain, kind in ((potsdam_chain((64, 64)), T.SamplePlan), (aug_chain((64, 64)), T.AugSamplePlan)):
        dp = T.DevicePlan(chain)
        _seed(5)
        p = dp.plan(80, 96)
        after = _states()
        assert type(p) is kind and dp.rot is None
        # the plan of the chain WITH the op carries exactly that tuple as its base when the turn's draws are taken away
        with_rot = list(chain[:-1]) + [T.RandomRot90(0.75), chain[-1]] if kind is T.SamplePlan else chain[:4] + [T.RandomRot90(0.75)] + chain[4:]
        dr = T.DevicePlan(with_rot)
        dr.rot.draw = lambda: 2
        _seed(5)
        q = dr.plan(80, 96)
        assert q == T.RotPlan(p, 2) and type(q.base) is kind and _same_state(after, _states()) and dr.extended == dp.extended
    assert type(T.DevicePlan([T.Normalize(T._MEAN, T._STD)]).plan(8, 8)) is T.SamplePlan


def test_other_positions_of_the_op_are_refused_by_name():
    for chain, name in ((lambda: rot_chain((64, 64))[:4] + [T.RandomDistort(hue_prob=0), T.RandomRot90(), T.Normalize()], "RandomRot90 at position 5"),
                        (lambda: [T.RandomRot90()] + potsdam_chain((64, 64)), "RandomRot90 at position 0"),
                        (lambda: potsdam_chain((64, 64))[:3] + [T.RandomRot90(), T.RandomVerticalFlip(), T.Normalize()], "RandomVerticalFlip at position 4")):
        with pytest.raises(ValueError, match=name):
            T.DevicePlan(chain())


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------------

def test_block_5_turns_have_the_promised_distribution():
    """8192 (step, sample) pairs at prob 0.75, key 1234: 64 steps of 128 samples.  Each of the four turns is expected 2048 times; the binomial
    standard deviation is sqrt(8192 * 1/4 * 3/4) = 39.19, so 4 sigma is 156.8.  Deterministic: key 1234 gives the counts [2043, 2002, 2132, 2015]
    (printed below), all inside."""
    turns = [t for step in range(64) for t in rot_turns(KEY, step, 0, 128, 0.75)]
    assert len(turns) == 8192
    four_sigma = 4.0 * math.sqrt(8192 * 0.25 * 0.75)
    counts = [turns.count(k) for k in range(4)]
    print("block-5 turns, key %d: %r (4 sigma = %.1f)" % (KEY, counts, four_sigma))
    assert 156 < four_sigma < 157 and sum(counts) == 8192
    for k, c in enumerate(counts):
        assert abs(c - 2048) <= four_sigma, (k, c)
    # a pure function of (key, step, rank * B + b): two ranks of 8 draw what one rank of 16 draws; prob 0 and 1
    assert rot_turns(KEY, 7, 0, 8, 0.75) + rot_turns(KEY, 7, 1, 8, 0.75) == rot_turns(KEY, 7, 0, 16, 0.75)
    assert rot_turns(KEY, 7, 0, 64, 0.0) == [0] * 64 and set(rot_turns(KEY, 7, 0, 64, 1.0)) == {1, 2, 3}
    assert rot_turns(KEY, 7, 0, 16, 0.75) != rot_turns(KEY, 8, 0, 16, 0.75) != rot_turns(KEY + (1 << 32), 8, 0, 16, 0.75)
    assert rot_turns(KEY, 7 + (1 << 32), 0, 16, 0.75) != rot_turns(KEY, 7, 0, 16, 0.75)


def test_the_turns_are_the_variant_codes_of_tta_d4_and_the_composite_is_uniform_on_d4():
    """Turn k is variant code TURN_CODES[k] of include/emrt_hip_tta.h.  Enumerating the chain's draws -- horizontal flip (probability 1/2), vertical
    flip (any probability v), turn (0 with 1/4, else 1..3 each 1/4 at ROT90_PROB 0.75) -- every one of the eight variants of --tta d4 comes out with
    probability exactly 1/8, whatever v is."""
    from fractions import Fraction
    from emrt_amd.src.api.scene import TTA_MODES
    a = np.arange(25).reshape(5, 5)
    for k in range(4):
        assert np.array_equal(np.rot90(a, k), variant(a, TURN_CODES[k])), k
    d4 = {code: variant(a, code).tobytes() for code in TTA_MODES["d4"]}
    assert len(set(d4.values())) == 8
    for v in (Fraction(0), Fraction(1, 10), Fraction(1, 2), Fraction(1)):
        mass = dict.fromkeys(d4.values(), Fraction(0))
        for h, vf, k in itertools.product((0, 1), (0, 1), range(4)):
            out = a[:, ::-1] if h else a
            out = out[::-1] if vf else out
            out = np.ascontiguousarray(np.rot90(out, k))
            mass[out.tobytes()] += Fraction(1, 2) * (v if vf else 1 - v) * Fraction(1, 4)
        assert set(mass) == set(d4.values()) and all(m == Fraction(1, 8) for m in mass.values()), (v, mass)


# ---- the library --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    from emrt_amd import build_ext
    build_ext.build(verbose=False)
    return build_ext.library("rot").lib


def test_rot_library_exports_exactly_what_its_header_declares(built):
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.ROT_HEADER)
    assert sorted(protos) == ["emrt_rot_batch", "emrt_rot_last_error", "emrt_rot_scene_batch", "emrt_rot_version"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in protos if n not in exported]
    assert not [n for n in exported if n.startswith("emrt_") and n not in protos]
    pinned = [_lib.parse_header()] + [_lib.parse_header(row.header) for row in _lib.SIDE_LIBRARIES.values()]
    assert len(pinned) == 6 and not any(set(protos) & set(p) for p in pinned)          # nothing is declared twice
    assert [len(p) for p in pinned] == [109, 6, 4, 7, 4, 4]                            # the six pinned headers are untouched
    assert _lib.parse_structs(_lib.ROT_HEADER) == {}


def test_rot_header_matches_its_definitions():
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.ROT_HEADER)
    defs = {}
    for f in glob.glob(os.path.join(ROOT, "emrt_amd/csrc/rot_ext/*.hip")):
        for m in re.finditer(r'extern "C" ([^{;]+?)\{', open(f).read(), re.S):
            p = re.sub(r"/\*.*?\*/", "", " ".join(m.group(1).split()))
            name = re.search(r"(\w+)\s*\(", p).group(1)
            args = p[p.index("(") + 1:p.rindex(")")]
            defs[name] = [] if args.strip() in ("", "void") else [re.match(r"(.*?)(\w+)$", " ".join(a.split())).group(1).strip() for a in args.split(",")]
    assert set(defs) == set(protos)
    for name, (ret, args) in protos.items():
        assert [t for t, _ in args] == defs[name], name


def test_the_second_list_of_libraries(built):
    """build_ext.LATER_LIBRARIES / _lib.LATER_SIDE_LIBRARIES continue the pinned tables: the same row types, built, hashed and looked up with them."""
    from emrt_amd import _lib, build_ext
    assert [os.path.basename(r.lib) for r in build_ext.LATER_LIBRARIES] == ["libemrt_hip_rot.so"] and list(_lib.LATER_SIDE_LIBRARIES) == ["rot"]
    assert not set(_lib.LATER_SIDE_LIBRARIES) & set(_lib.SIDE_LIBRARIES)
    digest = build_ext.source_digest()
    for row in build_ext.LATER_LIBRARIES:
        assert type(row) is build_ext.Library and build_ext.library(row.name) is row and row.header in build_ext._headers()
        assert all(os.path.exists(os.path.join(row.dir, s)) for s in row.sources)
        with open(row.lib + ".inputs") as f:
            assert os.path.exists(row.lib) and f.read().strip() == digest
        side = _lib.LATER_SIDE_LIBRARIES[row.name]
        assert type(side) is _lib.SideLibrary and (side.header, side.path) == (row.header, os.environ.get(side.env) or row.lib)
        assert hasattr(_lib, side.slot) and side.slot not in [s.slot for s in _lib.SIDE_LIBRARIES.values()]
    for row in build_ext.LIBRARIES:          # the library's stamp is the one digest of all seven
        with open(row.lib + ".inputs") as f:
            assert f.read().strip() == digest


def test_loader_of_the_rot_library(built, monkeypatch, tmp_path):
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_ROT_LIB", None)
    R = _lib.rot_lib()
    assert R.query("emrt_rot_version") == 1 and R is _lib.rot_lib() and R is _lib.side_lib("rot") and sorted(R.protos) == sorted(_lib.parse_header(_lib.ROT_HEADER))
    monkeypatch.setitem(_lib.LATER_SIDE_LIBRARIES, "rot", _lib.LATER_SIDE_LIBRARIES["rot"]._replace(path=str(tmp_path / "nope.so")))
    monkeypatch.setattr(_lib, "_ROT_LIB", None)
    with pytest.raises(_lib.EmrtHipError, match=r"nope\.so not found.*no CPU/PyTorch fallback for the quarter turn"):
        _lib.rot_lib()


def test_entry_points_refuse_bad_arguments_before_any_launch(built, monkeypatch):
    """Against the real library, no GPU: every bad call returns non-zero with a message naming the argument before anything touches a device.
    The device pointers are a made-up address, never dereferenced; the turns are a real host array, and it is what is checked."""
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_ROT_LIB", None)
    R = _lib.rot_lib()
    p = ctypes.c_void_p(0x10000)

    def refused(match, name, *args):
        with pytest.raises(_lib.EmrtHipError, match=match) as e:
            R.call(name, *args)
        assert "launch failed" not in str(e.value) and str(e.value).startswith(name + " failed")
        assert re.search(match, R.last_error())

    turns = lambda *v: (ctypes.c_int * len(v))(*v)
    refused(r"emrt_rot_batch: turns\[2\] is 4: a turn must be 0\.\.3", "emrt_rot_batch", p, p, turns(0, 3, 4), 3, 8, None)
    refused(r"emrt_rot_batch: turns\[0\] is -1: a turn must be 0\.\.3", "emrt_rot_batch", p, None, turns(-1), 1, 8, None)
    refused("emrt_rot_batch: n must be at least 1", "emrt_rot_batch", p, p, turns(1), 1, 0, None)
    refused("emrt_rot_batch: B must be at least 1", "emrt_rot_batch", p, p, turns(1), 0, 8, None)
    refused("emrt_rot_batch: n must be at most 32768", "emrt_rot_batch", p, p, turns(1), 1, 32769, None)
    refused("emrt_rot_batch: null pointer", "emrt_rot_batch", None, p, turns(1), 1, 8, None)
    refused("emrt_rot_batch: null pointer", "emrt_rot_batch", p, p, None, 1, 8, None)
    refused("emrt_rot_scene_batch: B must be 1..65535", "emrt_rot_scene_batch", p, 1, 0, 0, 8, 0.75, p, p, p, None)
    refused("emrt_rot_scene_batch: B must be 1..65535", "emrt_rot_scene_batch", p, 1, 0, 65536, 8, 0.75, p, p, p, None)
    refused("emrt_rot_scene_batch: n must be at least 1", "emrt_rot_scene_batch", p, 1, 0, 8, 0, 0.75, p, p, p, None)
    refused("emrt_rot_scene_batch: null pointer", "emrt_rot_scene_batch", None, 1, 0, 8, 8, 0.75, p, p, p, None)
    refused("emrt_rot_scene_batch: null pointer", "emrt_rot_scene_batch", p, 1, 0, 8, 8, 0.75, p, p, None, None)
    refused("rank \\* B \\+ b must fit", "emrt_rot_scene_batch", p, 1, -1, 8, 8, 0.75, p, p, p, None)
    refused("rank \\* B \\+ b must fit", "emrt_rot_scene_batch", p, 1, 1 << 30, 8, 8, 0.75, p, p, p, None)
    for prob in (-0.1, 1.5, float("nan")):
        refused(r"the rotation probability must be in \[0, 1\]", "emrt_rot_scene_batch", p, 1, 0, 8, 8, prob, p, p, p, None)


# ---- wiring on recording stand-ins --------------------------------------------------------------------------------------------------------------

class FakeRotLib(FakeAugLib):
    """Recording stand-in for libemrt_hip_rot.so: checks argument count and kinds against include/emrt_hip_rot.h, logs, computes nothing."""

    def __init__(self):
        from emrt_amd import _lib
        self.protos = _lib.parse_header(_lib.ROT_HEADER)
        self.calls = []


@pytest.fixture
def fakes(monkeypatch):
    from emrt_amd import _lib
    from tests import fake_abi
    main = fake_abi.install()
    aug, rot = FakeAugLib(), FakeRotLib()
    monkeypatch.setattr(_lib, "_AUG_LIB", aug)
    monkeypatch.setattr(_lib, "_ROT_LIB", rot)
    yield main, aug, rot
    fake_abi.uninstall()


SIZES = [(40, 56), (33, 47), (64, 64)]


def _first_batch(cfg, root, crop):
    from emrt_amd.distributed import DistributedTileSampler
    cfg.DATA.DATA_PATH = root
    cfg.DATA.CROP_SIZE = list(crop)
    ds = D.get_dataset(cfg, T.get_transforms(cfg), "train")
    _seed(3)
    before = set(threading.enumerate())
    gen = D.DeviceTileLoader(ds, DistributedTileSampler(len(ds), 4, 0, 1, shuffle=False, seed=2), "cpu", workers=1, prefetch=1).epochs()
    out = next(gen)
    gen.close()
    for t in set(threading.enumerate()) - before:          # random / np.random are process-global: a prefetching reader finishes its draws first
        t.join(timeout=10)
    return out


def test_the_default_key_never_asks_for_the_library(fakes, monkeypatch, tmp_path):
    """rot_lib() raises here: get_transforms, DevicePlan, a SceneSampler and its fill, and a DeviceTileLoader batch of the default and the augment
    chains go through without it, with the calls they make today."""
    from emrt_amd import _lib
    main, aug, rot = fakes
    monkeypatch.setattr(_lib, "_ROT_LIB", None)
    boom = lambda *a: (_ for _ in ()).throw(AssertionError("the default key loaded libemrt_hip_rot.so"))
    monkeypatch.setattr(_lib, "rot_lib", boom)
    monkeypatch.setattr(_lib, "_ExtLib", boom)
    root = str(tmp_path / "s")
    write_scene_tree(root, SIZES)
    bank = SceneBank(root, "cpu")
    images, labels = torch.empty(8, 3, 32, 32), torch.empty(8, 32, 32, dtype=torch.int64)
    for yaml, want_main, want_aug in (("EMRT_256x256_160k_potsdam.yaml", ["emrt_scene_draw", "emrt_scene_sample"], []),
                                      ("EMRT_256x256_160k_potsdam_augment.yaml", [], ["emrt_aug_scene_draw", "emrt_aug_scene_sample"])):
        cfg = _cfg(yaml)
        cfg.DATA.CROP_SIZE = (32, 32)
        chain = T.get_transforms(cfg)
        assert T.DevicePlan(chain).rot is None
        s = SceneSampler(bank, chain, 8, 1234, 3)
        assert s.turns is None and s.rot_prob == 0.0
        main.calls.clear(), aug.calls.clear()
        s.fill(images, labels)
        assert [n for n, _ in main.calls] == want_main and [n for n, _ in aug.calls] == want_aug
    tiles = _tile_tree(str(tmp_path / "p"), [(80, 96), (130, 70), (64, 64), (40, 100)])
    main.calls.clear(), aug.calls.clear()
    _first_batch(_cfg(), tiles, (96, 64))
    assert [n for n, _ in main.calls] == ["emrt_augment_tiles"] and aug.calls == []
    main.calls.clear()
    _first_batch(_cfg("EMRT_256x256_160k_potsdam_augment.yaml"), tiles, (96, 64))
    assert main.calls == [] and [n for n, _ in aug.calls] == ["emrt_aug_tiles"]
    assert _lib._ROT_LIB is None and rot.calls == []


@pytest.mark.parametrize("extended", [False, True])
def test_scene_sampler_appends_one_launch_after_the_sample_launch(fakes, tmp_path, monkeypatch, extended):
    from emrt_amd.runtime import ctx
    main, aug, rot = fakes
    root = str(tmp_path / "s")
    write_scene_tree(root, SIZES)
    bank = SceneBank(root, "cpu")
    images, labels = torch.empty(8, 3, 32, 32), torch.empty(8, 32, 32, dtype=torch.int64)
    chain = rot_chain((32, 32), vflip=0.25) if extended else rot_chain((32, 32), vflip=None, distort=False, rot=0.6)
    s = SceneSampler(bank, chain, 8, 0xFEDCBA9876543210, 3)
    assert s.turns.shape == (8,) and s.turns.dtype == torch.int32 and s.rot_prob == (0.75 if extended else 0.6)
    order = []
    for lib, tag in ((main, "main"), (aug, "aug"), (rot, "rot")):
        real = lib.call
        monkeypatch.setattr(lib, "call", lambda name, *a, _real=real, _tag=tag: (order.append((_tag, name)), _real(name, *a))[1])
    uploads = []
    real_to = torch.Tensor.to
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "to", lambda self, *a, **k: (uploads.append(a), real_to(self, *a, **k))[1])
        s.fill(images, labels)
    want = [("aug", "emrt_aug_scene_draw"), ("aug", "emrt_aug_scene_sample")] if extended else [("main", "emrt_scene_draw"), ("main", "emrt_scene_sample")]
    assert order == want + [("rot", "emrt_rot_scene_batch")] and uploads == []
    a = rot.calls[0][1]
    assert a[0].value == ctx().step_counter.data_ptr() and a[1] == 0xFEDCBA9876543210 - (1 << 64) and a[2:5] == (3, 8, 32) and a[5] == s.rot_prob
    assert a[6].value == images.data_ptr() and a[7].value == labels.data_ptr() and a[8].value == s.turns.data_ptr()
    with pytest.raises(ValueError, match="RandomRot90 needs a square crop"):
        SceneSampler(bank, rot_chain((40, 32)), 8, 1, 0)


def test_tile_loader_turns_the_batch_it_just_wrote(fakes, tmp_path):
    main, aug, rot = fakes
    tiles = _tile_tree(str(tmp_path / "p"), [(80, 96), (130, 70), (64, 64), (40, 100)])
    cfg = _cfg("EMRT_256x256_160k_potsdam_d4.yaml")
    main.calls.clear()
    out, lab = _first_batch(cfg, tiles, (64, 64))
    assert main.calls == [] and [n for n, _ in aug.calls] == ["emrt_aug_tiles"] and [n for n, _ in rot.calls] == ["emrt_rot_batch"]
    a = rot.calls[0][1]
    assert a[0].value == out.data_ptr() and a[1].value == lab.data_ptr() and a[3:5] == (4, 64) and out.shape == (4, 3, 64, 64)
    turns = list(a[2])
    # the turns are the ones a seeded DevicePlan draws for the same files in the same order
    _seed(3)
    dp = T.DevicePlan(T.get_transforms(cfg))
    assert turns == [dp.plan(h, w).turn for h, w in [(80, 96), (130, 70), (64, 64), (40, 100)]] and len(turns) == 4
    # without distortion and vertical flip: the main library's kernel, then the turn
    cfg = _cfg()
    cfg.DATA.AUGMENT.ROT90_PROB = 1.0
    aug.calls.clear(), rot.calls.clear()
    _first_batch(cfg, tiles, (24, 24))
    assert [n for n, _ in main.calls] == ["emrt_augment_tiles"] and aug.calls == [] and [n for n, _ in rot.calls] == ["emrt_rot_batch"]
    assert all(1 <= k <= 3 for k in rot.calls[0][1][2])
