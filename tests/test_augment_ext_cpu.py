"""CPU: RandomVerticalFlip and RandomDistort through every host layer, without a GPU.

  restatement   tests/distort_reference.py (plain numpy) equals PIL's ImageEnhance, bit for bit
  transforms    RandomDistort equals a literal PIL transcription of the reference under the same seeds and leaves random / np.random where it
                does; RandomVerticalFlip; the draw() helpers; hue is refused
  config        the DATA.AUGMENT keys, the chains they make, LoveDA's refusal, the augment yaml
  DevicePlan    the three extended chains, refusals by name, the same decisions and generator state as the CPU chain
  draws         the device draw procedure restated in Python (replay_aug; tests/test_gpu_augment_ext.py holds the kernel to it): distribution
  library       libemrt_hip_augment.so exports what include/emrt_hip_augment.h declares, the generated struct has the compiled layout, every
                host-side refusal returns non-zero with a message before any launch
  wiring        the loaders on a recording stand-in for the second library"""
import argparse
import ctypes
import glob
import itertools
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from emrt_amd.config import get_config, update_config
from emrt_amd.src import datasets as D
from emrt_amd.src import transforms as T
from emrt_amd.src.datasets import SceneBank, SceneSampler
from tests import distort_reference as R
from tests.test_scene_sampler_cpu import M32, below, philox4x32_10, potsdam_chain, potsdam_scales, replay, write_scene_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "emrt_amd/configs/EMRT")
OP_NAMES = ("brightness", "contrast", "saturation")
PIL_OPS = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}


def aug_chain(crop_wh, vflip=0.5, distort=True, pad=(0, 0, 0), label_pad=255, rng=0.4, prob=0.5):
    """The Potsdam chain with the augment yaml's extra ops; crop_wh = (w, h)."""
    extra = [T.RandomVerticalFlip(prob=vflip)] if vflip is not None else []
    if distort:
        extra.append(T.RandomDistort(rng, prob, rng, prob, rng, prob, hue_prob=0))
    return [T.ResizeStepScaling(0.5, 2.0, 0.25), T.RandomPaddingCrop(crop_size=crop_wh, img_padding_value=pad, label_padding_value=label_pad),
            T.RandomHorizontalFlip(prob=0.5)] + extra + [T.Normalize(mean=T._MEAN, std=T._STD)]


def replay_aug(key, step, rank, B, sizes, tile, crop, scales, prob, vprob, distort, ranges, probs):
    """The draws of emrt_aug_scene_draw, restated: B rows of 18 (include/emrt_hip_augment.h).  Columns 0-8 are emrt_scene_draw's."""
    k = (key & M32, (key >> 32) & M32)
    perms = list(itertools.permutations(range(4)))            # lexicographic
    rows = []
    for b, r in enumerate(replay(key, step, rank, B, sizes, tile, crop, scales, prob)):
        ctr = [step & M32, (step >> 32) & M32, (rank * B + b) & M32]
        r2, r3, r4 = (philox4x32_10(ctr + [j], k) for j in (2, 3, 4))
        vflip = int(r2[1] * 2.0 ** -32 < vprob)
        perm = below(r3[0], r3[1], 24)
        wp, wf = [r3[2], r4[0], r4[2]], [r3[3], r4[1], r4[3]]
        ops, bits = [], []
        for op in perms[perm]:
            if op < 3 and distort and wp[op] * 2.0 ** -32 < probs[op]:
                lower, upper = 1.0 - ranges[op], 1.0 + ranges[op]
                ops.append(op)
                bits.append(int(np.float32(lower + (upper - lower) * (wf[op] * 2.0 ** -32)).view(np.int32)))
        n = len(ops)
        rows.append(r[:9] + [vflip, perm, n] + ops + [0] * (3 - n) + bits + [0x3F800000] * (3 - n))
    return rows


def row_ops(row):
    """[(op name, float factor)] of a row of the extended draw table."""
    return [(OP_NAMES[row[12 + i]], float(np.int32(row[15 + i]).view(np.float32))) for i in range(row[11])]


def _states():
    return np.random.get_state(), random.getstate()


def _same_state(a, b):
    (na, ra), (nb, rb) = a, b
    return ra == rb and na[0] == nb[0] and np.array_equal(na[1], nb[1]) and na[2:] == nb[2:]


def _seed(s):
    np.random.seed(s)
    random.seed(s)


# ---- the restatement against PIL ----------------------------------------------------------------------------------------------------------------

def _images():
    g = np.random.RandomState(0)
    red = np.zeros((9, 11, 3), np.uint8)
    red[..., 0] = 255
    return [g.randint(0, 256, (37, 53, 3)).astype(np.uint8), np.zeros((9, 11, 3), np.uint8), np.full((9, 11, 3), 255, np.uint8), red]


@pytest.mark.parametrize("op", OP_NAMES)
def test_restatement_equals_pil(op):
    g = np.random.RandomState(1)
    r = 0.4
    factors = [1 - r, 1 + r, 1.0, 0.0] + g.uniform(1 - r, 1 + r, 200).tolist()
    for img in _images():
        pil = Image.fromarray(img)
        for f in factors:
            want = np.asarray(PIL_OPS[op](pil).enhance(f))
            assert np.array_equal(R.enhance(img, op, f), want), (op, f)


def test_blend_equals_pil_over_every_degenerate_and_value():
    """Image.blend on all 256 x 256 (degenerate, value) pairs at 50 factors, the float32 neighbours of 0 and 1 among them."""
    g = np.random.RandomState(2)
    one = np.float32(1.0)
    factors = [0.0, 1.0, float(np.nextafter(one, np.float32(0))), float(np.nextafter(one, np.float32(2))), float(np.nextafter(np.float32(0), one)),
               0.6, 1.4, 0.5, 1.5, 2.0] + g.uniform(0.0, 2.0, 40).tolist()
    assert len(factors) == 50
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    pd, px = Image.fromarray(d), Image.fromarray(x)
    for f in factors:
        want = np.asarray(Image.blend(pd, px, f))
        assert np.array_equal(R.blend(d.astype(np.int64), x.astype(np.int64), f), want), f


# ---- the transform classes ----------------------------------------------------------------------------------------------------------------------

def _reference_distort(img, br, bp, cr, cp, sr, sp, hr, hp):
    """transforms.py:621-681 with functional.py:76-96, transcribed: the draws and PIL calls of the reference (hue is never reached at hp = 0)."""
    def brightness(img, lower, upper):
        return ImageEnhance.Brightness(img).enhance(np.random.uniform(lower, upper))

    def contrast(img, lower, upper):
        return ImageEnhance.Contrast(img).enhance(np.random.uniform(lower, upper))

    def saturation(img, lower, upper):
        return ImageEnhance.Color(img).enhance(np.random.uniform(lower, upper))

    def hue(img, lower, upper):
        raise AssertionError("hue is off")

    ops = [brightness, contrast, saturation, hue]
    random.shuffle(ops)
    params = {"brightness": (1 - br, 1 + br), "contrast": (1 - cr, 1 + cr), "saturation": (1 - sr, 1 + sr), "hue": (-hr, hr)}
    probs = {"brightness": bp, "contrast": cp, "saturation": sp, "hue": hp}
    img = Image.fromarray(img.astype("uint8"))
    for op in ops:
        if np.random.uniform(0, 1) < probs[op.__name__]:
            img = op(img, *params[op.__name__])
    return np.asarray(img).astype("float32")


def test_random_distort_equals_the_pil_transcription_and_the_restatement():
    g = np.random.RandomState(3)
    img = (g.rand(29, 41, 3) * 255.99).astype(np.float32)             # fractional values: the uint8 truncation matters
    lab = g.randint(0, 6, (29, 41)).astype(np.uint8)
    args = (0.5, 0.5, 0.4, 0.7, 0.3, 0.6, 18, 0)
    t = T.RandomDistort(*args)
    orders = set()
    for seed in range(60):
        _seed(seed)
        want = _reference_distort(img, *args)
        after = _states()
        _seed(seed)
        got, got_lab = t(img, lab)
        assert got.dtype == np.float32 and np.array_equal(got, want) and got_lab is lab, seed
        assert _same_state(after, _states()), seed
        _seed(seed)
        ops = t.draw()                                                  # draw() alone leaves the generators where __call__ does
        assert _same_state(after, _states()), seed
        assert np.array_equal(T.RandomDistort.apply(img, ops), want) and np.array_equal(R.distort(img, ops), want), (seed, ops)
        orders.add(tuple(o for o, _ in ops))
        assert (t(img)[0].shape, len(t(img))) == (img.shape, 1)
    assert len(orders) > 8 and () in orders


def test_random_distort_refuses_hue():
    with pytest.raises(ValueError, match="hue"):
        T.RandomDistort()                                               # the reference's defaults: hue_range 18, hue_prob 0.5
    with pytest.raises(ValueError, match="hue"):
        T.RandomDistort(hue_prob=0.1, hue_range=5)
    t = T.RandomDistort(hue_prob=0)
    assert (t.brightness_range, t.brightness_prob, t.contrast_range, t.contrast_prob, t.saturation_range, t.saturation_prob, t.hue_range) == (
        0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 18)


def test_random_vertical_flip():
    g = np.random.RandomState(4)
    img, lab = g.rand(7, 9, 3).astype(np.float32), g.randint(0, 6, (7, 9)).astype(np.uint8)
    assert T.RandomVerticalFlip().prob == 0.1
    t = T.RandomVerticalFlip(prob=0.5)
    flips = 0
    for seed in range(40):
        random.seed(seed)
        want = random.random() < 0.5
        after = random.getstate()
        random.seed(seed)
        gi, gl = t(img, lab)
        assert random.getstate() == after
        assert np.array_equal(gi, img[::-1] if want else img) and np.array_equal(gl, lab[::-1] if want else lab)
        random.seed(seed)
        assert t.draw() == want and random.getstate() == after
        flips += want
    assert 5 < flips < 35 and len(t(img)) == 1


# ---- config -------------------------------------------------------------------------------------------------------------------------------------

def _cfg(name="EMRT_256x256_160k_potsdam.yaml"):
    cfg = update_config(get_config(), argparse.Namespace(cfg=os.path.join(CFG_DIR, name)))
    cfg.defrost()
    return cfg


def _params(t):
    return type(t).__name__, {k: (tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in vars(t).items()}


def test_default_keys_leave_the_chains_as_they_were():
    aug = get_config().DATA.AUGMENT
    assert aug.VFLIP_PROB == 0.0 and dict(aug.DISTORT) == {
        "ENABLE": False, "BRIGHTNESS_RANGE": 0.4, "CONTRAST_RANGE": 0.4, "SATURATION_RANGE": 0.4, "BRIGHTNESS_PROB": 0.5, "CONTRAST_PROB": 0.5,
        "SATURATION_PROB": 0.5}
    for name in ("EMRT_256x256_160k_potsdam.yaml", "EMRT_256x256_120k_vaihingen.yaml"):
        cfg = _cfg(name)
        assert [_params(t) for t in T.get_transforms(cfg)] == [_params(t) for t in potsdam_chain((256, 256))]
    assert [_params(t) for t in T.get_transforms(_cfg("EMRT_256x256_160k_loveda.yaml"))] == [_params(T.Normalize(mean=T._MEAN, std=T._STD))]


def test_each_key_inserts_its_op_at_the_stated_position():
    names = lambda cfg: [type(t).__name__ for t in T.get_transforms(cfg)]
    head, tail = ["ResizeStepScaling", "RandomPaddingCrop", "RandomHorizontalFlip"], ["Normalize"]
    cfg = _cfg()
    cfg.DATA.AUGMENT.VFLIP_PROB = 0.25
    assert names(cfg) == head + ["RandomVerticalFlip"] + tail and T.get_transforms(cfg)[3].prob == 0.25
    cfg = _cfg("EMRT_256x256_120k_vaihingen.yaml")
    cfg.DATA.AUGMENT.DISTORT.ENABLE = True
    cfg.DATA.AUGMENT.DISTORT.CONTRAST_RANGE = 0.3
    cfg.DATA.AUGMENT.DISTORT.SATURATION_PROB = 0.9
    assert names(cfg) == head + ["RandomDistort"] + tail
    d = T.get_transforms(cfg)[3]
    assert (d.brightness_range, d.brightness_prob, d.contrast_range, d.contrast_prob, d.saturation_range, d.saturation_prob, d.hue_prob) == (
        0.4, 0.5, 0.3, 0.5, 0.4, 0.9, 0)
    cfg.DATA.AUGMENT.VFLIP_PROB = 0.5
    assert names(cfg) == head + ["RandomVerticalFlip", "RandomDistort"] + tail


def test_loveda_refuses_either_key():
    cfg = _cfg("EMRT_256x256_160k_loveda.yaml")
    cfg.DATA.AUGMENT.VFLIP_PROB = 0.5
    with pytest.raises(ValueError, match=r"DATA\.AUGMENT\.VFLIP_PROB.*LoveDA"):
        T.get_transforms(cfg)
    cfg.DATA.AUGMENT.VFLIP_PROB = 0.0
    cfg.DATA.AUGMENT.DISTORT.ENABLE = True
    with pytest.raises(ValueError, match=r"DATA\.AUGMENT\.DISTORT\.ENABLE.*LoveDA"):
        T.get_transforms(cfg)


def test_the_augment_yaml_parses_and_unknown_keys_are_refused(tmp_path):
    cfg = _cfg("EMRT_256x256_160k_potsdam_augment.yaml")
    assert cfg.DATA.DATASET == "Potsdam" and cfg.DATA.AUGMENT.VFLIP_PROB == 0.5 and cfg.DATA.AUGMENT.DISTORT.ENABLE is True
    assert [_params(t) for t in T.get_transforms(cfg)] == [_params(t) for t in aug_chain((256, 256))]
    bad = tmp_path / "bad.yaml"
    bad.write_text("DATA: {AUGMENT: {ROTATE_PROB: 0.5}}\n")
    with pytest.raises(KeyError, match=r"DATA\.AUGMENT\.ROTATE_PROB"):
        update_config(get_config(), argparse.Namespace(cfg=str(bad)))


# ---- DevicePlan ---------------------------------------------------------------------------------------------------------------------------------

def _forced(chain, p):
    """The chain with its draws replaced by the plan's decisions (no RNG call)."""
    from tests.test_device_transforms_cpu import _scale_for
    chain[0].draw = lambda: _scale_for(chain[0], p)
    chain[1].draw = lambda ih, iw: None if (ih, iw) == chain[1].size() else (p.off_y, p.off_x)
    chain[2].draw = lambda: bool(p.flip)
    for t in chain[3:-1]:
        if isinstance(t, T.RandomVerticalFlip):
            t.draw = lambda: bool(p.vflip)
        else:
            t.draw = lambda: list(p.ops)
    return T.Compose(chain)


@pytest.mark.parametrize("vflip,distort", [(0.5, False), (None, True), (0.5, True)])
@pytest.mark.parametrize("src,crop", [((80, 96), (64, 64)), ((37, 41), (64, 48)), ((64, 64), (64, 64))])
def test_planner_draws_the_extended_chains_decisions(vflip, distort, src, crop):
    """Per seed: the CPU chain, then (same seed) DevicePlan.plan: the same generator state afterwards, and the chain re-run with its draws forced
    to the plan's decisions gives the same arrays."""
    H, W = src
    g = np.random.RandomState(H * 1000 + W)
    img = g.randint(0, 256, (H, W, 3)).astype(np.float32)
    lab = g.randint(0, 6, (H, W)).astype(np.uint8)
    chain = lambda: aug_chain(crop, vflip=vflip, distort=distort)
    dp = T.DevicePlan(chain())
    assert dp.extended and (dp.vflip is not None) == (vflip is not None) and (dp.distort is not None) == distort
    seen = set()
    for seed in range(40):
        _seed(seed)
        want_img, want_lab = T.Compose(chain())(img, lab)
        after = _states()
        _seed(seed)
        p = dp.plan(H, W)
        assert isinstance(p, T.AugSamplePlan) and _same_state(after, _states()), (seed, p)
        got_img, got_lab = _forced(chain(), p)(img, lab)
        assert np.array_equal(want_img, got_img) and np.array_equal(want_lab, got_lab), (seed, p)
        seen.add((p.vflip, len(p.ops)))
    assert dp.out_size(H, W) == (crop[1], crop[0])
    assert {v for v, _ in seen} == ({0, 1} if vflip else {0}) and ({n for _, n in seen} > {0} if distort else {n for _, n in seen} == {0})


def test_todays_chains_keep_their_plan():
    dp = T.DevicePlan(potsdam_chain((64, 64)))
    _seed(5)
    p = dp.plan(80, 96)
    assert type(p) is T.SamplePlan and len(p) == 7 and not dp.extended
    assert not T.DevicePlan([T.Normalize(T._MEAN, T._STD)]).extended


@pytest.mark.parametrize("chain,name", [
    (lambda: aug_chain((64, 64))[:3] + [T.RandomDistort(hue_prob=0), T.RandomVerticalFlip(), T.Normalize()], "RandomVerticalFlip at position 4"),
    (lambda: [T.RandomVerticalFlip()] + potsdam_chain((64, 64)), "RandomVerticalFlip at position 0"),
    (lambda: aug_chain((64, 64))[:2] + [T.RandomVerticalFlip(), T.RandomHorizontalFlip(), T.Normalize()], "RandomVerticalFlip at position 2"),
    (lambda: [T.RandomDistort(hue_prob=0), T.Normalize()], "RandomDistort at position 0"),
    (lambda: aug_chain((64, 64))[:5], "chain ends early"),
])
def test_other_orders_are_refused_by_name(chain, name):
    with pytest.raises(ValueError, match=name):
        T.DevicePlan(chain())


def test_distort_parameters_the_device_cannot_run_are_refused():
    with pytest.raises(ValueError, match="img_padding_value must lie in"):
        T.DevicePlan(aug_chain((64, 64), pad=(300, 0, 0)))
    chain = aug_chain((64, 64))
    chain[4].contrast_range = 1.5                                       # a negative factor could be drawn
    with pytest.raises(ValueError, match="contrast_range"):
        T.DevicePlan(chain)


# ---- the draw procedure -------------------------------------------------------------------------------------------------------------------------

def test_replay_aug_has_the_promised_distribution():
    """7000 samples: each of the 24 permutations, each op's apply rate and the vertical flip within 5 binomial standard deviations; factors inside
    their ranges and in both outer 5 % bands; the first nine columns are emrt_scene_draw's."""
    sizes, tile = [(40, 56), (33, 47), (64, 64)], (32, 32)
    scales = potsdam_scales(tile)
    ranges, probs = [0.4, 0.3, 0.2], [0.5, 0.3, 0.8]
    rows = []
    for step in range(7):
        got = replay_aug(1234, step, 0, 1000, sizes, tile, tile, scales, 0.5, 0.25, True, ranges, probs)
        assert [r[:9] for r in got] == [r[:9] for r in replay(1234, step, 0, 1000, sizes, tile, tile, scales, 0.5)]
        rows += got
    n = len(rows)
    assert n == 7000 and all(len(r) == 18 for r in rows)
    five_sigma = lambda p: 5.0 * math.sqrt(n * p * (1.0 - p))
    for perm in range(24):
        cnt = sum(r[10] == perm for r in rows)
        assert abs(cnt - n / 24) <= five_sigma(1 / 24), (perm, cnt)
    assert abs(sum(r[9] for r in rows) - n * 0.25) <= five_sigma(0.25)
    perms = list(itertools.permutations(range(4)))
    for op in range(3):
        fs = [f for r in rows for (name, f) in row_ops(r) if name == OP_NAMES[op]]
        assert abs(len(fs) - n * probs[op]) <= five_sigma(probs[op]), (op, len(fs))
        lo, hi = 1 - ranges[op], 1 + ranges[op]
        width = hi - lo
        assert float(np.float32(lo)) <= min(fs) < lo + 0.05 * width and hi - 0.05 * width < max(fs) <= float(np.float32(hi)), (op, min(fs), max(fs))
    for r in rows:      # the applied ops keep the permutation's order, hue dropped; unused slots hold op 0 and factor 1.0
        applied = [r[12 + i] for i in range(r[11])]
        order = [o for o in perms[r[10]] if o in applied]
        assert applied == order and len(set(applied)) == len(applied)
        assert all(r[12 + i] == 0 and r[15 + i] == 0x3F800000 for i in range(r[11], 3))
    # distortion off: the same flips and permutation, no op
    off = replay_aug(1234, 0, 0, 1000, sizes, tile, tile, scales, 0.5, 0.25, False, ranges, probs)
    assert [r[:11] for r in off] == [r[:11] for r in rows[:1000]] and all(r[11:] == [0, 0, 0, 0] + [0x3F800000] * 3 for r in off)


# ---- the second library -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    from emrt_amd import build_ext
    build_ext.build(verbose=False)
    return build_ext.library("augment").lib


def test_second_library_exports_exactly_what_its_header_declares(built):
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.AUG_HEADER)
    assert sorted(protos) == ["emrt_aug_last_error", "emrt_aug_scene_draw", "emrt_aug_scene_sample", "emrt_aug_tiles", "emrt_aug_version",
                              "emrt_aug_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [n for n in protos if n not in exported]
    assert not [n for n in exported if n.startswith("emrt_") and n not in protos]
    assert not set(protos) & set(_lib.parse_header())                   # nothing is declared twice; the main header is untouched
    assert len(_lib.parse_header()) == 109


def test_second_header_matches_its_definitions():
    from emrt_amd import _lib
    protos = _lib.parse_header(_lib.AUG_HEADER)
    defs = {}
    files = glob.glob(os.path.join(ROOT, "emrt_amd/csrc/augment_ext/*.hip"))
    assert files
    for f in files:
        for m in re.finditer(r'extern "C" ([^{;]+?)\{', open(f).read(), re.S):
            p = re.sub(r"/\*.*?\*/", "", " ".join(m.group(1).split()))
            name = re.search(r"(\w+)\s*\(", p).group(1)
            args = p[p.index("(") + 1:p.rindex(")")]
            defs[name] = [] if args.strip() in ("", "void") else [re.match(r"(.*?)(\w+)$", " ".join(a.split())).group(1).strip() for a in args.split(",")]
    assert set(defs) == set(protos)
    for name, (ret, args) in protos.items():
        assert [t for t, _ in args] == defs[name], name


def test_generated_struct_has_the_compiled_layout(tmp_path):
    from emrt_amd import _lib
    from tests.test_abi_cpu import _host_cxx
    structs = _lib.parse_structs(_lib.AUG_HEADER)
    assert list(structs) == ["EmrtAugOpsDesc"]
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "emrt_hip_augment.h"', "int main() {"]
    for name, members in structs.items():
        lines.append('  std::printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  std::printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, m, name, m) for _, m, _ in members]
    (tmp_path / "layout.cpp").write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([_host_cxx(), "-std=c++17", "-I", os.path.dirname(_lib.AUG_HEADER), str(tmp_path / "layout.cpp"), "-o", exe], check=True,
                   capture_output=True, text=True)
    compiled = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    S = _lib.augment_struct("EmrtAugOpsDesc")
    generated = {"EmrtAugOpsDesc": str(ctypes.sizeof(S))}
    generated.update({"EmrtAugOpsDesc.%s" % m: str(getattr(S, m).offset) for _, m, _ in structs["EmrtAugOpsDesc"]})
    assert generated == compiled and len(generated) == 1 + 12
    assert S is _lib.augment_struct("EmrtAugOpsDesc") and set(_lib.parse_structs()) & set(structs) == set()
    with pytest.raises(_lib.EmrtHipError, match="EmrtNoSuchDesc"):
        _lib.augment_struct("EmrtNoSuchDesc")


def test_loader_of_the_second_library(built, monkeypatch, tmp_path):
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_AUG_LIB", None)
    A = _lib.augment_lib()
    assert A.query("emrt_aug_version") == 1 and A.query("emrt_aug_workspace_bytes", 17) == 17 * 8
    assert A.query("emrt_aug_workspace_bytes", 0) == 0 and "B must be positive" in A.last_error()
    monkeypatch.setitem(_lib.SIDE_LIBRARIES, "augment", _lib.SIDE_LIBRARIES["augment"]._replace(path=str(tmp_path / "nope.so")))
    monkeypatch.setattr(_lib, "_AUG_LIB", None)
    with pytest.raises(_lib.EmrtHipError, match="not found"):
        _lib.augment_lib()


def test_entry_points_refuse_bad_arguments_before_any_launch(built, monkeypatch):
    """Against the real library, no GPU: every bad call returns non-zero with a message before anything touches a device.  The device pointers are
    a made-up address, never dereferenced; descriptors and host mirrors are real arrays, and they are what is checked."""
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "_AUG_LIB", None)
    A = _lib.augment_lib()
    Desc = _lib.augment_struct("EmrtAugOpsDesc")
    p = ctypes.c_void_p(0x10000)
    mean, sinv = (ctypes.c_double * 3)(1, 2, 3), (ctypes.c_double * 3)(1, 1, 1)

    def desc(n_ops=1, op=(1, 0, 0), factor=(1.2, 1.0, 1.0), flip=0, H=40, W=56, h=40, w=56, img_off=0, lab_off=3 * 40 * 56, off_y=0):
        d = Desc(img_off, lab_off, H, W, h, w, off_y, 0, flip, n_ops)
        for k in range(3):
            d.op[k], d.factor[k] = op[k], factor[k]
        return d

    def tiles(match, d=None, B=1, OH=32, distort=1, pad=(0, 0, 0), src=p, out=p, ws=p, ws_bytes=8, label_pad=255, src_bytes=4 * 40 * 56):
        descs = (Desc * 1)(d if d is not None else desc())
        with pytest.raises(_lib.EmrtHipError, match=match):
            A.call("emrt_aug_tiles", src, src_bytes, descs, B, OH, 32, distort, mean, sinv, (ctypes.c_float * 3)(*pad), label_pad, None, out, 3 * OH * 32,
                   p, ws, ws_bytes, None)

    # (every case below must fail a check: one that passed would launch on the made-up pointers)
    tiles("emrt_aug_tiles: null pointer", src=None)
    tiles("null pointer", out=None)
    tiles("positive", B=0)
    tiles("positive", OH=0)
    tiles("descriptor 0: op code must be", d=desc(op=(3, 0, 0)))
    tiles("descriptor 0: op code must be", d=desc(op=(-1, 0, 0)))
    tiles("descriptor 0: an op appears twice", d=desc(n_ops=2, op=(2, 2, 0)))
    tiles("descriptor 0: factors must be finite and >= 0", d=desc(factor=(-0.5, 1, 1)))
    tiles("factors must be finite", d=desc(factor=(float("nan"), 1, 1)))
    tiles("factors must be finite", d=desc(factor=(float("inf"), 1, 1)))
    tiles("n_ops must be 0..3", d=desc(n_ops=4))
    tiles("n_ops must be 0..3", d=desc(n_ops=-1))
    tiles("colour ops need distort", distort=0)
    tiles("flip must be a mask", d=desc(flip=4))
    tiles("sizes must be positive", d=desc(h=0))
    tiles("crop outside the padded image", d=desc(off_y=9))
    tiles("image outside the staged buffer", src_bytes=3 * 40 * 56 - 1)
    tiles("label map outside the staged buffer", src_bytes=4 * 40 * 56 - 1)
    tiles("workspace smaller than", ws_bytes=7)
    tiles("null pointer \\(workspace\\)", ws=None)
    tiles("img_pad must lie in", pad=(0, 256, 0))
    tiles("img_pad must lie in", pad=(-1, 0, 0))
    tiles("label_pad", label_pad=256)

    H, W = 40, 56
    good = [(0, 3 * H * W, H, W), (4 * H * W, 4 * H * W + 3 * 64 * 64, 64, 64)]
    nbytes = 4 * H * W + 4 * 64 * 64
    scale_hw = (ctypes.c_int * 32)(*([32, 32] * 16))

    def entries(rows):
        return (D._SceneEntry * len(rows))(*[D._SceneEntry(*r) for r in rows])

    def cum_of(rows, th, tw):
        c = [0]
        for _, _, h, w in rows:
            c.append(c[-1] + (h - th + 1) * (w - tw + 1))
        return c

    def draw(match, rows=good, cum=None, th=32, B=8, n_scales=7, prob=0.5, vprob=0.5, ranges=(0.4, 0.4, 0.4), probs=(0.5, 0.5, 0.5), step=p, draws=p,
             bank_bytes=nbytes, rank=0):
        host = entries(rows)
        c = cum_of(rows, th, 32) if cum is None else cum
        with pytest.raises(_lib.EmrtHipError, match=match):
            A.call("emrt_aug_scene_draw", step, p, p, host, (ctypes.c_longlong * len(c))(*c), len(rows), bank_bytes, 1234, rank, B, th, 32, 32, 32, prob, vprob,
                   1, None if ranges is None else (ctypes.c_double * 3)(*ranges), None if probs is None else (ctypes.c_double * 3)(*probs), scale_hw,
                   n_scales, draws, None)

    draw("emrt_aug_scene_draw: null pointer", step=None)
    draw("null pointer", draws=None)
    draw("null pointer", ranges=None)
    draw("null pointer", probs=None)
    draw("positive", B=0)
    draw("1 to 16 scale entries", n_scales=17)
    draw("the flip probability must be in \\[0, 1\\]", prob=1.5)
    draw("vertical flip probability must be in \\[0, 1\\]", vprob=1.01)
    draw("vertical flip probability", vprob=float("nan"))
    draw("op probability must be in \\[0, 1\\]", probs=(0.5, 1.5, 0.5))
    draw("op probability", probs=(-0.1, 0.5, 0.5))
    draw("op range must be in \\[0, 1\\]", ranges=(0.4, -0.1, 0.4))
    draw("op range", ranges=(0.4, 0.4, 1.5))
    draw("op range", ranges=(float("nan"), 0.4, 0.4))
    draw("32-bit counter word", rank=1 << 30)
    draw("scene 0: the 41x32 tile is larger than the 40x56 scene", th=41, cum=[0, 1, 2])
    draw("scene 1: image or label map outside the bank", bank_bytes=nbytes - 1)
    draw("not increasing at scene 1", cum=[0, 225, 225])
    draw("must start at 0", cum=[1, 226, 1315])

    def sample(match, rows=good, th=32, B=8, bank=p, out=p, draws=p, distort=1, ws=p, ws_bytes=64, pad=(0, 0, 0), bank_bytes=nbytes, OH=32):
        with pytest.raises(_lib.EmrtHipError, match=match):
            A.call("emrt_aug_scene_sample", bank, bank_bytes, p, entries(rows), len(rows), draws, B, th, 32, OH, 32, distort, mean, sinv,
                   (ctypes.c_float * 3)(*pad), 255, None, out, 3 * OH * 32, p, ws, ws_bytes, None)

    sample("emrt_aug_scene_sample: null pointer", bank=None)
    sample("null pointer", out=None)
    sample("null pointer", draws=None)
    sample("B must be", B=0)
    sample("positive", OH=0)
    sample("workspace smaller than", ws_bytes=63)
    sample("null pointer \\(workspace\\)", ws=None)
    sample("img_pad must lie in", pad=(0, 0, 300))
    sample("scene 0: the 41x32 tile is larger than the 40x56 scene", th=41)
    sample("scene 1: image or label map outside the bank", bank_bytes=nbytes - 1)
    sample("n_scenes must be positive", rows=[])


# ---- host wiring on a recording stand-in --------------------------------------------------------------------------------------------------------

class FakeAugLib:
    """Recording stand-in for libemrt_hip_augment.so: checks argument count and kinds against include/emrt_hip_augment.h, logs, computes nothing."""

    def __init__(self):
        from emrt_amd import _lib
        self.protos = _lib.parse_header(_lib.AUG_HEADER)
        self.calls = []

    def _check(self, name, args):
        spec = self.protos[name][1]
        assert len(args) == len(spec), "%s: %d args given, header declares %d" % (name, len(args), len(spec))
        for a, (t, an) in zip(args, spec):
            if t.endswith("*"):
                assert a is None or isinstance(a, (ctypes.c_void_p, int, ctypes.Array)), "%s.%s: bad pointer %r" % (name, an, a)
            elif t in ("float", "double"):
                assert isinstance(a, (int, float)) and not isinstance(a, bool), "%s.%s: expected a number, got %r" % (name, an, a)
            else:
                assert isinstance(a, int) and not isinstance(a, bool), "%s.%s (%s): expected int, got %r" % (name, an, t, a)

    def call(self, name, *args):
        self._check(name, args)
        self.calls.append((name, args))

    def query(self, name, *args):
        self._check(name, args)
        return {"emrt_aug_version": 1, "emrt_aug_workspace_bytes": 8 * args[0] if args else 0}[name]

    def last_error(self):
        return ""


@pytest.fixture
def fakes(monkeypatch):
    from emrt_amd import _lib
    from tests import fake_abi
    main = fake_abi.install()
    aug = FakeAugLib()
    monkeypatch.setattr(_lib, "_AUG_LIB", aug)
    yield main, aug
    fake_abi.uninstall()


SIZES = [(40, 56), (33, 47), (64, 64)]


def test_scene_sampler_wiring(fakes, tmp_path, monkeypatch):
    main, aug = fakes
    root = str(tmp_path / "s")
    write_scene_tree(root, SIZES)
    bank = SceneBank(root, "cpu")
    images, labels = torch.empty(8, 3, 32, 32), torch.empty(8, 32, 32, dtype=torch.int64)
    # today's chain: today's two entry points, nothing on the second library
    plain = SceneSampler(bank, potsdam_chain((32, 32)), 8, 1234, 3)
    assert plain.draws.shape == (8, 10)
    main.calls.clear()
    plain.fill(images, labels)
    assert [n for n, _ in main.calls] == ["emrt_scene_draw", "emrt_scene_sample"] and aug.calls == []
    # an extended chain: the second library's two entry points, <= 4 launches in all (draw; memset + statistics + apply), and no upload
    s = SceneSampler(bank, aug_chain((32, 32), vflip=0.25, rng=0.3, prob=0.6), 8, 1234, 3)
    assert s.draws.shape == (8, 18) and s.draws.dtype == torch.int32 and s.vflip_prob == 0.25 and s.flip_prob == 0.5
    main.calls.clear()
    uploads = []
    real_to = torch.Tensor.to
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "to", lambda self, *a, **k: (uploads.append(a), real_to(self, *a, **k))[1])
        m.setattr(torch, "from_numpy", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fill() made a host array into a tensor")))
        s.fill(images, labels)
    assert uploads == [] and main.calls == [] and [n for n, _ in aug.calls] == ["emrt_aug_scene_draw", "emrt_aug_scene_sample"]
    d, a = aug.calls[0][1], aug.calls[1][1]
    scenes_dev, cum_dev, scenes_host, cum_host = bank.tables(32, 32)
    assert d[1].value == scenes_dev.data_ptr() and d[3].value == ctypes.addressof(scenes_host) and d[4].value == ctypes.addressof(cum_host)
    assert d[5:17] == (3, bank.nbytes, 1234, 3, 8, 32, 32, 32, 32, 0.5, 0.25, 1)
    assert [ctypes.cast(d[17], ctypes.POINTER(ctypes.c_double))[i] for i in range(3)] == [0.3] * 3
    assert [ctypes.cast(d[18], ctypes.POINTER(ctypes.c_double))[i] for i in range(3)] == [0.6] * 3
    assert d[20] == 7 and d[21].value == s.draws.data_ptr()
    assert a[0].value == bank.buffer.data_ptr() and a[5].value == s.draws.data_ptr() and a[6:12] == (8, 32, 32, 32, 32, 1)
    assert a[15] == 255 and a[17].value == images.data_ptr() and a[18] == 3 * 32 * 32 and a[19].value == labels.data_ptr()
    assert a[20].value == s._ws.data_ptr() and a[21] == 64 and s._ws.numel() * 8 == 64
    # a flip alone: no distortion, the same two entry points with distort = 0
    aug.calls.clear()
    v = SceneSampler(bank, aug_chain((32, 32), vflip=1.0, distort=False), 8, 1234, 0)
    v.fill(images, labels)
    assert aug.calls[0][1][15:17] == (1.0, 0) and aug.calls[1][1][11] == 0


def _tile_tree(root, sizes):
    rng = np.random.RandomState(0)
    for sub in ("train", "test"):
        os.makedirs(os.path.join(root, sub))
        os.makedirs(os.path.join(root, sub + "_convert_labels"))
        for i, (h, w) in enumerate(sizes):
            Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, sub, "%d.tif" % i))
            Image.fromarray(rng.randint(0, 6, (h, w), dtype=np.uint8)).save(os.path.join(root, sub + "_convert_labels", "%d.png" % i))
    return root


def test_tile_loader_wiring(fakes, tmp_path):
    from emrt_amd import _lib
    from emrt_amd.distributed import DistributedTileSampler
    main, aug = fakes
    root = _tile_tree(str(tmp_path / "p"), [(80, 96), (130, 70), (64, 64), (40, 100)])

    def first_batch(yaml):
        cfg = _cfg(yaml)
        cfg.DATA.DATA_PATH = root
        cfg.DATA.CROP_SIZE = [96, 64]
        ds = D.get_dataset(cfg, T.get_transforms(cfg), "train")
        _seed(3)
        gen = D.DeviceTileLoader(ds, DistributedTileSampler(len(ds), 4, 0, 1, shuffle=False, seed=2), "cpu", workers=1, prefetch=1).epochs()
        out = next(gen)
        gen.close()
        return out

    main.calls.clear()
    first_batch("EMRT_256x256_160k_potsdam.yaml")
    assert [n for n, _ in main.calls] == ["emrt_augment_tiles"] and aug.calls == []
    main.calls.clear()
    out, lab = first_batch("EMRT_256x256_160k_potsdam_augment.yaml")
    assert main.calls == [] and [n for n, _ in aug.calls] == ["emrt_aug_tiles"]
    a = aug.calls[0][1]
    assert out.shape == (4, 3, 64, 96) and lab.shape == (4, 64, 96) and a[3:7] == (4, 64, 96, 1) and a[10] == 255 and a[13] == 3 * 64 * 96
    descs = a[2]
    assert isinstance(descs, ctypes.Array) and descs._type_ is _lib.augment_struct("EmrtAugOpsDesc") and len(descs) == 4
    for d_ in descs:
        assert 0 <= d_.flip <= 3 and 0 <= d_.n_ops <= 3 and len({d_.op[k] for k in range(d_.n_ops)}) == d_.n_ops
        assert all(0.6 <= d_.factor[k] <= 1.4 for k in range(d_.n_ops)) and all(d_.factor[k] == 1.0 for k in range(d_.n_ops, 3))
    assert a[16] == 32 and a[15].value is not None
