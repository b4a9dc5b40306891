"""CPU: the device-side tile sampler of `train.py --data scenes` without a GPU.  Philox4x32-10 and the whole draw procedure of emrt_scene_draw
are restated here in pure Python (`philox4x32_10`, `replay`): the restatement reproduces the Random123 known answers, its draws have the
distribution the procedure promises, and tests/test_gpu_scene_sampler.py holds the kernel to it bit for bit.  SceneBank's packing and refusals,
the entry points' argument checks and SceneSampler's two launches are checked against the real library (no launch) and the recording ABI."""
import argparse
import ctypes
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from emrt_amd.config import get_config, update_config
from emrt_amd.src import datasets as D
from emrt_amd.src import transforms as T
from emrt_amd.src.datasets import SceneBank, SceneSampler, label_lut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "emrt_amd/configs/EMRT/EMRT_256x256_160k_potsdam.yaml")
M32 = 0xFFFFFFFF

SIZES = [(40, 56), (33, 47), (64, 64)]          # the bank of the distribution check and of every GPU test
TILE = CROP = (32, 32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): 4 counter words, 2 key words -> 4 words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def below(lo, hi, n):
    """Uniform integer below n from two output words: the high 64 bits of ((hi << 32) | lo) * n."""
    return (((hi << 32) | lo) * n) >> 64


def potsdam_scales(tile, lo=0.5, hi=2.0, step=0.25):
    """The scale table the host builds for the Potsdam chain: ResizeStepScaling.resized over its np.linspace factors."""
    n = int((hi - lo) / step + 1)
    return [T.ResizeStepScaling.resized(f, tile[0], tile[1]) for f in np.linspace(lo, hi, n).tolist()]


def replay(key, step, rank, B, sizes, tile, crop, scales, prob):
    """The draws of emrt_scene_draw, restated: -> B rows [scene, y0, x0, scale_index, h, w, off_y, off_x, flip, 0]."""
    th, tw = tile
    OH, OW = crop
    cum = [0]
    for H, W in sizes:
        cum.append(cum[-1] + (H - th + 1) * (W - tw + 1))
    k = (key & M32, (key >> 32) & M32)
    rows = []
    for b in range(B):
        ctr = [step & M32, (step >> 32) & M32, (rank * B + b) & M32]
        r0, r1, r2 = (philox4x32_10(ctr + [j], k) for j in range(3))
        g = below(r0[0], r0[1], cum[-1])
        scene = max(i for i in range(len(sizes)) if cum[i] <= g)
        rem, nx = g - cum[scene], sizes[scene][1] - tw + 1
        si = below(r0[2], r0[3], len(scales))
        h, w = scales[si]
        off_y = below(r1[0], r1[1], max(h, OH) - OH + 1)
        off_x = below(r1[2], r1[3], max(w, OW) - OW + 1)
        flip = int(r2[0] * 2.0 ** -32 < prob)
        rows.append([scene, rem // nx, rem % nx, si, h, w, off_y, off_x, flip, 0])
    return rows


def write_scene_tree(root, sizes, ncls=6, seed=0, sub=("images", "labels"), names=None, label_values=None):
    """A scene tree written with PIL: <root>/images/<name>.tif (RGB) + <root>/labels/<name>.png (uint8 class indices) -> [(img, lab)] arrays."""
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, sub[0]), exist_ok=True)
    os.makedirs(os.path.join(root, sub[1]), exist_ok=True)
    out = []
    for i, (H, W) in enumerate(sizes):
        name = names[i] if names else "scene_%d" % i
        img = rng.randint(0, 256, (H, W, 3), dtype=np.uint8)
        lab = rng.randint(0, ncls, (H, W), dtype=np.uint8) if label_values is None else rng.choice(np.asarray(label_values, np.uint8), (H, W))
        lab[rng.rand(H, W) < 0.05] = 255
        Image.fromarray(img).save(os.path.join(root, sub[0], name + ".tif"))
        Image.fromarray(lab).save(os.path.join(root, sub[1], name + ".png"))
        out.append((img, lab))
    return out


def potsdam_chain(crop_hw):
    return [T.ResizeStepScaling(0.5, 2.0, 0.25), T.RandomPaddingCrop(crop_size=(crop_hw[1], crop_hw[0]), img_padding_value=(0, 0, 0), label_padding_value=255),
            T.RandomHorizontalFlip(prob=0.5), T.Normalize(mean=T._MEAN, std=T._STD)]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([M32] * 4, [M32] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_restatement_reproduces_the_random123_known_answers(counter, key, want):
    assert " ".join("%08x" % v for v in philox4x32_10(counter, key)) == want


def test_replay_is_a_pure_function_of_key_step_rank_and_sample():
    scales = potsdam_scales(TILE)
    a = replay(1234, 7, 1, 8, SIZES, TILE, CROP, scales, 0.5)
    assert a == replay(1234, 7, 1, 8, SIZES, TILE, CROP, scales, 0.5)
    # rank r's sample b is sample r * B + b of the step: two ranks of 8 draw what one rank of 16 draws
    both = replay(1234, 7, 0, 16, SIZES, TILE, CROP, scales, 0.5)
    assert replay(1234, 7, 0, 8, SIZES, TILE, CROP, scales, 0.5) + a == both
    for other in (replay(1235, 7, 1, 8, SIZES, TILE, CROP, scales, 0.5), replay(1234, 8, 1, 8, SIZES, TILE, CROP, scales, 0.5),
                  replay(1234, 7 + (1 << 32), 1, 8, SIZES, TILE, CROP, scales, 0.5), replay(1234 + (1 << 32), 7, 1, 8, SIZES, TILE, CROP, scales, 0.5)):
        assert other != a


def test_replay_has_the_promised_distribution():
    """7000 samples (7 steps of 1000) over the three-scene bank with the Potsdam chain: every count within 5 binomial standard deviations of its
    expectation, every extreme origin and offset reached, no offset where the resized tile does not exceed the crop.  Seeded: deterministic."""
    scales = potsdam_scales(TILE)
    assert scales == [(16, 16), (24, 24), (32, 32), (40, 40), (48, 48), (56, 56), (64, 64)]
    rows = [r for step in range(7) for r in replay(1234, step, 0, 1000, SIZES, TILE, CROP, scales, 0.5)]
    n = len(rows)
    assert n == 7000
    five_sigma = lambda p: 5.0 * math.sqrt(n * p * (1.0 - p))
    assert five_sigma(1 / 7) < 147
    for k in range(7):
        cnt = sum(r[3] == k for r in rows)
        assert abs(cnt - 1000) <= five_sigma(1 / 7), (k, cnt)
    origins = [(H - TILE[0] + 1) * (W - TILE[1] + 1) for H, W in SIZES]
    assert origins == [225, 32, 1089] and sum(origins) == 1346
    for s, o in enumerate(origins):
        p = o / 1346
        cnt = sum(r[0] == s for r in rows)
        assert abs(cnt - n * p) <= five_sigma(p), (s, cnt, n * p)
    flips = sum(r[8] for r in rows)
    assert abs(flips - n / 2) <= five_sigma(0.5), flips
    for s, (H, W) in enumerate(SIZES):
        ys, xs = {r[1] for r in rows if r[0] == s}, {r[2] for r in rows if r[0] == s}
        assert min(ys) == 0 and max(ys) == H - TILE[0] and min(xs) == 0 and max(xs) == W - TILE[1], (s, sorted(ys), sorted(xs))
    for k, (h, w) in enumerate(scales):
        oy, ox = {r[6] for r in rows if r[3] == k}, {r[7] for r in rows if r[3] == k}
        assert all((r[4], r[5]) == (h, w) for r in rows if r[3] == k)
        if h <= CROP[0]:
            assert oy == {0} and ox == {0}, (k, oy, ox)
        else:
            assert min(oy) == 0 and max(oy) == h - CROP[0] and min(ox) == 0 and max(ox) == w - CROP[1], (k, sorted(oy), sorted(ox))
    assert all(r[9] == 0 for r in rows)


def test_replay_reaches_origins_beyond_32_bits_of_precision():
    """A real bank has more than 2^30 origins: the reduction is the high half of a 64 x 64-bit product, so every origin of a 40000 x 40000
    scene can be drawn (a 32-bit multiply-shift could not reach the odd ones) and the largest is the last origin."""
    n = (40000 - 255) * (40000 - 255)
    assert n > 1 << 30
    assert below(M32, M32, n) == n - 1 and below(0, 0, n) == 0
    # n < 2^32: one step of the high word moves the result by 0 or 1, so no origin is skipped
    for hi in (0, 1, 0x7FFFFFFF, 0x9abcdef0, M32 - 1):
        assert below(0, hi + 1, n) - below(0, hi, n) in (0, 1)


# ---- SceneBank ----------------------------------------------------------------------------------------------------------------------------------

def test_scene_bank_packs_scenes_and_builds_tables(tmp_path):
    root = str(tmp_path / "s")
    names = ["b_top", "a_left", "c_mid"]
    arrays = dict(zip(names, write_scene_tree(root, SIZES, names=names)))
    bank = SceneBank(root, "cpu")
    assert bank.names == sorted(names) and len(bank) == 3            # name order, each image with the label map of its own name
    off = 0
    for name, (H, W), (io, lo) in zip(bank.names, bank.sizes, bank.offsets):
        img, lab = arrays[name]
        assert (H, W) == img.shape[:2] and (io, lo) == (off, off + 3 * H * W)
        assert np.array_equal(bank.buffer[io:lo].numpy().reshape(H, W, 3), img)
        assert np.array_equal(bank.buffer[lo:lo + H * W].numpy().reshape(H, W), lab)
        off += 4 * H * W
    assert bank.nbytes == off == bank.buffer.numel() and bank.buffer.dtype == torch.uint8
    scenes_dev, cum_dev, scenes_host, cum_host = bank.tables(32, 32)
    want = [(H - 31) * (W - 31) for H, W in bank.sizes]
    assert list(cum_host) == [0] + list(np.cumsum(want)) and cum_dev.dtype == torch.int64 and cum_dev.tolist() == list(cum_host)
    assert [(e.img_off, e.lab_off, e.H, e.W) for e in scenes_host] == [(io, lo, H, W) for (io, lo), (H, W) in zip(bank.offsets, bank.sizes)]
    assert ctypes.sizeof(D._SceneEntry) == 24 and scenes_dev.numpy().tobytes() == bytes(scenes_host)     # the device table is the host mirror
    assert bank.origins(24, 40) == [(H - 23) * (W - 39) for H, W in bank.sizes]
    with pytest.raises(ValueError, match=r"34x32 tile is larger than scene 0 \(a_left, 33x47\)"):
        bank.origins(34, 32)


def test_scene_bank_refusals(tmp_path, monkeypatch):
    root = str(tmp_path / "s")
    write_scene_tree(root, SIZES)
    os.remove(os.path.join(root, "labels", "scene_1.png"))
    with pytest.raises(FileNotFoundError, match=r"scene_1\.tif has no label map named scene_1"):
        SceneBank(root, "cpu")
    Image.fromarray(np.zeros((33, 48), np.uint8)).save(os.path.join(root, "labels", "scene_1.png"))
    with pytest.raises(ValueError, match=r"scene_1\.tif is 33x47 but its label map .*scene_1\.png is 33x48"):
        SceneBank(root, "cpu")
    Image.fromarray(np.zeros((33, 47), np.uint8)).save(os.path.join(root, "labels", "scene_1.png"))
    SceneBank(root, "cpu")
    Image.fromarray(np.zeros((33, 47), np.uint8)).save(os.path.join(root, "images", "scene_1.tif"))
    with pytest.raises(ValueError, match=r"scene_1\.tif is a L image; the bank holds 8-bit RGB"):
        SceneBank(root, "cpu")
    Image.fromarray(np.zeros((33, 47, 3), np.uint8)).save(os.path.join(root, "images", "scene_1.tif"))
    Image.fromarray(np.zeros((33, 47, 3), np.uint8)).save(os.path.join(root, "labels", "scene_1.png"))
    with pytest.raises(ValueError, match=r"scene_1\.png is a RGB image; label maps are uint8 class indices"):
        SceneBank(root, "cpu")
    Image.fromarray(np.zeros((33, 47), np.uint8)).save(os.path.join(root, "labels", "scene_1.png"))
    need = 4 * sum(H * W for H, W in SIZES)
    monkeypatch.setattr(D, "_free_device_bytes", lambda device: need - 1)
    with pytest.raises(MemoryError, match="needs %d bytes, the device has %d bytes free" % (need, need - 1)):
        SceneBank(root, "cpu")
    monkeypatch.setattr(D, "_free_device_bytes", lambda device: need)
    assert SceneBank(root, "cpu").nbytes == need
    with pytest.raises(FileNotFoundError, match="no directory"):
        SceneBank(str(tmp_path / "nowhere"), "cpu")


# ---- the entry points' checks -------------------------------------------------------------------------------------------------------------------

def _entries(rows):
    return (D._SceneEntry * len(rows))(*[D._SceneEntry(*r) for r in rows])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Against the real library, no GPU: every bad call returns non-zero with a message before anything touches a device.  The device pointers
    are a made-up address and never dereferenced; the host mirrors are real arrays, and they are what is checked."""
    from emrt_amd import _lib, build_ext
    build_ext.build(verbose=False)
    _lib._LIB = None
    L = _lib.lib()
    p = ctypes.c_void_p(0x10000)
    H, W = 40, 56
    good = [(0, 3 * H * W, H, W), (4 * H * W, 4 * H * W + 3 * 64 * 64, 64, 64)]
    nbytes = 4 * H * W + 4 * 64 * 64
    mean, sinv, pad = (ctypes.c_double * 3)(1, 2, 3), (ctypes.c_double * 3)(1, 1, 1), (ctypes.c_float * 3)(0, 0, 0)
    scale_hw = (ctypes.c_int * 32)(*([32, 32] * 16))

    def cum_of(rows, th, tw):
        c = [0]
        for _, _, h, w in rows:
            c.append(c[-1] + (h - th + 1) * (w - tw + 1))
        return c

    def draw(match, rows=good, cum=None, th=32, tw=32, B=8, n_scales=7, prob=0.5, bank_bytes=nbytes, step=p, dev=p, draws=p, scales=scale_hw, rank=0, OH=32):
        host = _entries(rows)
        c = cum_of(rows, th, tw) if cum is None else cum
        cum_host = (ctypes.c_longlong * len(c))(*c)
        with pytest.raises(_lib.EmrtHipError, match=match):
            L.call("emrt_scene_draw", step, dev, p, host, cum_host, len(rows), bank_bytes, 1234, rank, B, th, tw, OH, 32, prob, scales, n_scales, draws, None)

    def sample(match, rows=good, th=32, tw=32, B=8, bank_bytes=nbytes, bank=p, out=p, draws=p, labels=p, label_pad=255, OH=32):
        host = _entries(rows)
        with pytest.raises(_lib.EmrtHipError, match=match):
            L.call("emrt_scene_sample", bank, bank_bytes, p, host, len(rows), draws, B, th, tw, OH, 32, mean, sinv, pad, label_pad, None, out, 3 * OH * 32,
                   labels, None)

    # (every case below must fail a check: one that passed would launch on the made-up pointers)
    draw("emrt_scene_draw: null pointer", step=None)
    draw("null pointer", dev=None)
    draw("null pointer", draws=None)
    draw("null pointer", scales=None)
    draw("positive", B=0)
    draw("positive", B=-3)
    draw("positive", OH=0)
    draw("1 to 16 scale entries", n_scales=17)
    draw("1 to 16 scale entries", n_scales=0)
    draw("flip probability must be in \\[0, 1\\]", prob=1.5)
    draw("flip probability", prob=-0.01)
    draw("flip probability", prob=float("nan"))
    draw("32-bit counter word", rank=1 << 30, B=8)
    draw("scene 0: the 41x32 tile is larger than the 40x56 scene", th=41, cum=[0, 1, 2])
    draw("scene 1: the 32x65 tile is larger than the 64x64 scene", rows=[(0, 3 * 80 * 80, 80, 80), good[1]], tw=65, bank_bytes=1 << 20, cum=[0, 1, 2])
    draw("scene 1: image or label map outside the bank", bank_bytes=nbytes - 1)
    draw("scene 0: image or label map outside the bank", rows=[(-1, 3 * H * W, H, W)])
    draw("scene 0: image or label map outside the bank", rows=[(nbytes - 3 * H * W + 1, 0, H, W)])
    draw("scene 0: sizes must be positive", rows=[(0, 0, 0, W)], cum=[0, 1])
    draw("cumulative origin table is not increasing at scene 1", cum=[0, 225, 225])
    draw("not increasing at scene 0", cum=[0, 0, 1089])
    draw("must start at 0", cum=[1, 226, 1315])
    draw("scene 1: the cumulative origin table holds 1088 origins, the scene and tile sizes give 1089", cum=[0, 225, 225 + 1088])
    draw("scale entry 2: sizes must be", scales=(ctypes.c_int * 32)(*([32, 32, 16, 16, 0, 8] + [32] * 26)))

    sample("emrt_scene_sample: null pointer", bank=None)
    sample("null pointer", out=None)
    sample("null pointer", draws=None)
    sample("B must be", B=0)
    sample("positive", OH=0)
    sample("label_pad", label_pad=256)
    sample("scene 0: the 41x32 tile is larger than the 40x56 scene", th=41)
    sample("scene 1: image or label map outside the bank", bank_bytes=nbytes - 1)
    sample("n_scenes must be positive", rows=[])


# ---- SceneSampler through the recording ABI -----------------------------------------------------------------------------------------------------

@pytest.fixture
def fake():
    from tests import fake_abi
    f = fake_abi.install()
    yield f
    fake_abi.uninstall()


def test_sampler_issues_draw_then_sample_with_the_headers_arguments(fake, tmp_path):
    root = str(tmp_path / "s")
    write_scene_tree(root, SIZES)
    bank = SceneBank(root, "cpu")
    s = SceneSampler(bank, potsdam_chain(CROP), batch_size=8, seed=1234, rank=3)
    assert s.tile == s.crop == (32, 32) and s.scales == potsdam_scales(TILE) and s.flip_prob == 0.5 and s.lut is None
    assert s.key == 1234 and s.total_origins == 1346 and s.batch_shape == (8, 32, 32)
    assert s.draws.shape == (8, 10) and s.draws.dtype == torch.int32
    images, labels = torch.empty(8, 3, 32, 32), torch.empty(8, 32, 32, dtype=torch.int64)
    fake.calls.clear()
    s.fill(images, labels)
    assert [n for n, _ in fake.calls] == ["emrt_scene_draw", "emrt_scene_sample"]       # (fake_abi checks count and types against the header)
    from emrt_amd import runtime
    d = fake.calls[0][1]
    scenes_dev, cum_dev, scenes_host, cum_host = bank.tables(32, 32)
    assert d[0].value == runtime.ctx().step_counter.data_ptr() and d[1].value == scenes_dev.data_ptr() and d[2].value == cum_dev.data_ptr()
    assert d[3].value == ctypes.addressof(scenes_host) and d[4].value == ctypes.addressof(cum_host)
    assert d[5:15] == (3, bank.nbytes, 1234, 3, 8, 32, 32, 32, 32, 0.5)
    assert d[16] == 7 and [ctypes.cast(d[15], ctypes.POINTER(ctypes.c_int))[i] for i in range(14)] == [v for hw in s.scales for v in hw]
    assert d[17].value == s.draws.data_ptr()
    a = fake.calls[1][1]
    assert a[0].value == bank.buffer.data_ptr() and a[1] == bank.nbytes and a[4] == 3 and a[5].value == s.draws.data_ptr()
    assert a[6:11] == (8, 32, 32, 32, 32) and a[14] == 255 and a[15] is None
    assert [ctypes.cast(a[11], ctypes.POINTER(ctypes.c_double))[i] for i in range(3)] == T._MEAN
    assert [ctypes.cast(a[12], ctypes.POINTER(ctypes.c_double))[i] for i in range(3)] == list(1.0 / np.asarray(T._STD, dtype=np.float64))
    assert a[16].value == images.data_ptr() and a[17] == 3 * 32 * 32 and a[18].value == labels.data_ptr()
    with pytest.raises(ValueError, match="images must be contiguous fp32"):
        s.fill(images[:4], labels)
    with pytest.raises(ValueError, match="labels must be contiguous int64"):
        s.fill(images, labels.int())
    # a seed above 2^63 travels as the same 64 bits
    big = SceneSampler(bank, potsdam_chain(CROP), 8, (1 << 64) - 2, 0)
    fake.calls.clear()
    big.fill(images, labels)
    assert big.key == (1 << 64) - 2 and fake.calls[0][1][7] == -2
    # a non-square crop (w, h) = (40, 24): tile and crop are (h, w)
    ns = SceneSampler(bank, potsdam_chain((24, 40)), 2, 0, 0)
    assert ns.tile == (24, 40) and ns.scales[0] == (12, 20) and ns.scales[-1] == (48, 80)
    with pytest.raises(ValueError, match="24x48 tile is larger than scene 1"):
        SceneSampler(bank, potsdam_chain((24, 48)), 2, 0, 0)


def test_sampler_runs_lovedas_chain_as_one_scale_no_flip_and_the_shifted_lut(fake, tmp_path):
    root = str(tmp_path / "s")
    write_scene_tree(root, SIZES, label_values=[0, 1, 2, 3, 4, 5, 6, 7])
    bank = SceneBank(root, "cpu", label_shift=1)
    with pytest.raises(ValueError, match="needs the tile size"):
        SceneSampler(bank, [T.Normalize(mean=T._MEAN, std=T._STD)], 4, 1, 0)
    s = SceneSampler(bank, [T.Normalize(mean=T._MEAN, std=T._STD)], 4, 1, 0, tile=(32, 32))
    assert s.scales == [(32, 32)] and s.flip_prob == 0.0 and np.array_equal(s.lut, label_lut(1))
    fake.calls.clear()
    s.fill(torch.empty(4, 3, 32, 32), torch.empty(4, 32, 32, dtype=torch.int64))
    d, a = fake.calls[0][1], fake.calls[1][1]
    assert d[14] == 0.0 and d[16] == 1
    lut = ctypes.cast(a[15], ctypes.POINTER(ctypes.c_ubyte))
    assert [lut[i] for i in range(256)] == label_lut(1).tolist() and lut[0] == 255 and lut[1] == 0 and lut[255] == 255


@pytest.mark.parametrize("chain,name", [
    (lambda: [T.Resize(64), T.Normalize()], "Resize at position 0"),
    (lambda: [T.ResizeStepScaling(), T.RandomPaddingCrop((64, 64)), T.Normalize()], "Normalize at position 2"),
    (lambda: [], "chain ends early"),
])
def test_sampler_refuses_unsupported_chains_with_the_device_plans_message(tmp_path, chain, name):
    root = str(tmp_path / "s")
    write_scene_tree(root, SIZES)
    bank = SceneBank(root, "cpu")
    with pytest.raises(ValueError) as e:
        SceneSampler(bank, chain(), 2, 0, 0)
    with pytest.raises(ValueError) as want:
        T.DevicePlan(chain())
    assert str(e.value) == str(want.value) and name in str(e.value)


def test_sampler_refuses_a_continuous_scale():
    class _Bank:
        device, label_shift = torch.device("cpu"), 0
    chain = potsdam_chain(CROP)
    chain[0] = T.ResizeStepScaling(0.5, 2.0, 0)
    with pytest.raises(ValueError, match="scale_step_size 0"):
        SceneSampler(_Bank(), chain, 2, 0, 0)


# ---- engine and CLI -----------------------------------------------------------------------------------------------------------------------------

def test_scenes_and_device_transforms_are_refused_together():
    from emrt_amd import train
    with pytest.raises(SystemExit, match="--device_transforms cannot be combined with --data scenes"):
        train.main(["--data", "scenes", "--device_transforms"])


def test_engine_step_arguments_follow_the_batch_source():
    """The argument contract of TrainEngine.step, checked before anything is launched: tensors with a source, or none without, are refused."""
    from emrt_amd.engine import TrainEngine
    eng = TrainEngine.__new__(TrainEngine)
    eng.batch_source, eng.images, eng.labels = object(), torch.empty(1), torch.empty(1)
    with pytest.raises(ValueError, match="takes no tensors"):
        eng.step(torch.empty(1), torch.empty(1))
    eng.batch_source = None
    with pytest.raises(ValueError, match="images and labels are required"):
        eng.step()


def test_make_fake_scenes_writes_a_tree_the_bank_reads(tmp_path):
    import subprocess
    import sys
    root = str(tmp_path / "fake")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools/make_fake_scenes.py"), root, "--scenes", "2", "--size", "48", "--val", "1"], check=True)
    bank = SceneBank(root, "cpu")
    assert len(bank) == 2 and bank.sizes == [(48, 48)] * 2
    assert len(os.listdir(os.path.join(root, "val_images"))) == 1 == len(os.listdir(os.path.join(root, "val_labels")))
    cfg = update_config(get_config(), argparse.Namespace(cfg=CFG))
    val = D.SceneVal(T.get_val_transforms(cfg), root, 6)
    img, lab = val[0]
    assert img.shape[0] == 3 and img.dtype == np.float32 and lab.shape == (1, 48, 48)
