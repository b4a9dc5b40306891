"""The case lists of tests/fuzz_cases.py, checked without a GPU: every case is inside its entry point's accepted domain, every regime of
the sweeps keeps its cases, the ids are unique and stable, and the regime table of the module's docstring is the one the predicates give."""
import pytest

from tests import fuzz_cases as fc

OPS = sorted(fc.CASES)


@pytest.mark.parametrize("op", OPS)
def test_every_case_is_inside_the_accepted_domain(op):
    cases = fc.CASES[op]
    assert cases, op
    ids = [c[0] for c in cases]
    assert len(set(ids)) == len(ids)
    for c in cases:
        assert fc.IN_DOMAIN[op](c), "%s: %r is an expected refusal, not a case" % (op, c)


@pytest.mark.parametrize("op,regime", [(op, name) for op in OPS for name, _ in fc.REGIMES[op]])
def test_every_regime_keeps_its_cases(op, regime):
    ids = dict(fc.regime_hits(op))[regime]
    need = fc.REGIME_MIN.get((op, regime), 2)
    assert len(ids) >= need, "%s / %s: %d case(s) %s, need %d -- a seed or a range was edited" % (op, regime, len(ids), ids, need)


def test_the_generators_are_deterministic():
    assert fc.bn_cases() == fc.CASES["batchnorm"] and fc.resize_cases() == fc.CASES["resize"] and fc.ln_cases() == fc.CASES["layernorm"]


def test_case_sizes_stay_small():
    """the float64 CPU reference is the cost of a case"""
    for c in fc.CASES["batchnorm"]:
        assert c[1] * c[2] * c[3] * c[4] <= fc.MAX_ELEMS and 8 <= c[1] * c[2] * c[3] <= 600
    for c in fc.CASES["groupnorm"]:
        assert c[1] * c[2] * c[3] * c[4] <= fc.MAX_ELEMS
    for c in fc.CASES["groupnorm_levels"]:
        assert c[1] * sum(c[2]) * c[3] <= fc.MAX_ELEMS
    for c in fc.CASES["layernorm"]:
        assert c[1] * c[2] * c[3] <= fc.MAX_ELEMS and c[1] * c[2] <= 700
    for c in fc.CASES["resize"]:
        assert c[1] * max(c[2] * c[3], c[5] * c[6]) * c[4] <= fc.MAX_ELEMS
    for c in fc.CASES["maxpool"]:
        assert c[1] * c[2] * c[3] * c[4] <= fc.MAX_ELEMS
    for c in fc.CASES["adaptive_pool"]:
        assert c[1] * c[2] * c[3] * c[5] <= fc.MAX_ELEMS
    for c in fc.CASES["pyramid"]:
        assert c[1] * c[4] * c[5] * c[2] * (len(c[3]) + 1) <= fc.MAX_ELEMS
    for c in fc.CASES["mha"]:
        assert c[1] * c[2] * c[3] * c[3] <= fc.MAX_ELEMS and 1 <= c[1] <= 4 and c[2] in fc.MHA_MS and c[3] in fc.MHA_LS
    for c in fc.CASES["msda"]:          # its own cap: the smallest pyramid the row-band kernels take has Lv ~ 2500
        assert c[1] * max(fc.msda_lq(c), sum(h * w for h, w in c[3])) * c[2] * 32 <= fc.MSDA_MAX_ELEMS
    long_cases = []
    for c in fc.CASES["gconv"]:         # the three grid-stride cases have their own cap, the largest of their own tensors
        C, OC, _, _, M, Mi = fc.gconv_dims(c)
        hits = [name for name, pred in fc.GCONV_REGIMES if name.startswith("grid-stride") and pred(c)]
        assert max(Mi * C, M * OC) <= (fc.GCONV_LONG_MAX_ELEMS if hits else fc.MAX_ELEMS), c[0]
        if hits:
            long_cases.append(max(Mi * C, M * OC))
    assert len(long_cases) == 3 and max(long_cases) == fc.GCONV_LONG_MAX_ELEMS <= 17000000
    for c in fc.CASES["conv"]:          # every tensor with its padding, and the weight
        if c[11] in ("fwd", "bwd"):
            assert max(v.bs * c[1] for v in fc.conv_tensors(c).values()) <= fc.MAX_ELEMS and c[4] * c[5] * c[6] * c[6] <= fc.MAX_ELEMS, c[0]
            assert fc.conv_gemm_dims(c)[0] * fc.conv_gemm_dims(c)[1] * (c[6] * c[6] * (c[4] if c[11] == "fwd" else c[5])) <= 60000000, c[0]      # multiply-adds of the float64 reference


def test_loss_step_and_areas_case_sizes():
    """the seven cases that send a loss backward kernel or an optimizer kernel round its grid-stride loop a second time (and the one areas
    case past its 1024 blocks) have caps of their own; everything else stays below MAX_ELEMS"""
    long_cases = []
    for c in fc.CASES["loss"]:
        elems, hits = c[3] * c[4] * c[5] * c[6], fc._ls_bwd_twice(c)
        assert elems <= (fc.LOSS_LONG_MAX_ELEMS if hits else fc.MAX_ELEMS), c[0]
        long_cases += [c[0]] if elems > fc.MAX_ELEMS else []
    assert len(long_cases) == 4
    for c in fc.CASES["step"]:
        hits = fc._st_quads(c) > (fc.clip_grid(c[2]) if c[1] == "clip" else fc.step_grid(c[2])) * 256
        assert c[2] <= (fc.STEP_LONG_MAX_ELEMS if hits else fc.MAX_ELEMS), c[0]
        long_cases += [c[0]] if c[2] > fc.MAX_ELEMS else []
    assert len(long_cases) == 7 and fc.STEP_LONG_MAX_ELEMS == 8388615 and fc.LOSS_LONG_MAX_ELEMS == 2 * 1049600
    big = [c for c in fc.CASES["areas"] if c[4] > fc.MAX_ELEMS]
    assert len(big) == 1 and big[0][4] == fc.AREAS_LONG_MAX_ELEMS and all(c[4] <= 4097 for c in fc.CASES["areas"] if c is not big[0])


def test_loss_sweep_covers_what_it_was_written_for():
    """one assertion per gap the sweep was written to close in csrc/loss.hip, csrc/loss_pixel.hpp and csrc/loss_ext/loss_ext.hip"""
    cases = fc.CASES["loss"]
    assert fc.loss_cases() == cases and 50 <= len(cases) <= 64 and [c[0] for c in cases] == ["loss-%d" % i for i in range(len(cases))]
    fam = lambda f: [c for c in cases if c[1] == f]
    # each backward kernel goes round its loop a second time once, at 1 x 2 x 1025 x 1024, and there alone
    twice = [c for c in cases if fc._ls_bwd_twice(c)]
    assert [(c[1], c[2], c[10] != "none") for c in twice] == [("ce", "single", False), ("wce", "pair", True), ("ohem", "pair", False), ("dice", "pair", False)]
    assert all(c[3:7] == (1, 2, 1025, 1024) and fc.loss_depth(fc.loss_npix(c), fc.loss_grids(c)[1]) == 2 for c in twice)
    # the forward grids (1024 blocks) stride in every family, the OHEM histograms (128 blocks) in a case of ordinary size too
    for f in fc.LOSS_FAMILIES:
        assert any(fc.loss_npix(c) > 262144 and fc.loss_grids(c)[0] == 1024 for c in fam(f)), f
    assert any(32768 < fc.loss_npix(c) <= fc.MAX_ELEMS // c[4] and fc.loss_grids(c)[2] == 128 for c in fam("ohem"))
    # class counts, in every family that takes them (the Dice entry points stop at 64 classes)
    for f in ("ce", "wce", "ohem"):
        assert {1, 2, 3, 6, 7, 8, 9, 16, 17, 19, 150} - {c[4] for c in fam(f)} <= {1, 2, 3, 6, 7, 8, 9} and {16, 17, 19, 150} <= {c[4] for c in fam(f)}, f
    assert {1, 2, 8, 9, 16, 17, 19} <= {c[4] for c in fam("dice")} and {fc.lx_chunks(c[4]) for c in fam("dice")} == {1, 2, 3}
    assert {1, 2, 3, 6, 7, 8, 9, 16, 17, 19, 150} == {c[4] for c in cases}
    # pixel counts around a block, below a wave, and a block across two images of odd size, in every family
    for f in fc.LOSS_FAMILIES:
        assert {1, 15, 255, 256, 257} <= {fc.loss_npix(c) for c in fam(f)}, f
        assert any(c[3] >= 2 and (c[5] * c[6]) % 2 == 1 and c[5] * c[6] > 256 for c in fam(f)), f
        assert {"none", "tenth", "all", "allbut1", "oneclass"} == {c[8] for c in fam(f)}, f
        assert {255, -100} <= {c[7] for c in fam(f)} and any(0 <= c[7] < c[4] for c in fam(f)), f
        assert {"ordinary", "confident", "shift+", "shift-", "wide", "constant"} <= {c[9] for c in fam(f)}, f
        assert any(min(c[11]) < 0 for c in fam(f)) and any(0.0 in c[11] for c in fam(f)) and any(c[12] for c in fam(f)), f
    for f in ("wce", "dice"):
        assert {"random", "onezero", "zeropresent"} <= {c[10] for c in fam(f)}, f
    assert any(c[9] == "grid" for c in fam("ohem")) and {0, 1} <= {c[14] for c in fam("ohem")}
    # a label outside [0, C) that is not the ignore index is outside the contract: no pattern draws one, and a row that names one is refused
    assert not fc.loss_in_domain(cases[5][:8] + ("outside",) + cases[5][9:])
    assert not fc.loss_in_domain(cases[45][:4] + (65,) + cases[45][5:]) and not fc.loss_in_domain(cases[2][:7] + (1,) + cases[2][8:])


def test_step_sweep_covers_what_it_was_written_for():
    cases = fc.CASES["step"]
    assert fc.step_cases() == cases and 30 <= len(cases) <= 44
    upd = [c for c in cases if c[1] != "clip"]
    ns = {c[2] for c in cases}
    assert {1, 3, 4, 5} <= ns and {4 * q + t for q in (1023, 1024, 1025) for t in range(4)} <= ns
    for e in ("clip", "sgd", "adamw"):
        assert {1, 3, 4, 5} <= {c[2] for c in cases if c[1] == e}, e
    assert [c[2] for c in cases if c[1] == "clip" and c[2] > fc.MAX_ELEMS] == [4 * (2048 * 256 + 1) + 3]
    assert [(c[1], c[2]) for c in upd if c[2] > fc.MAX_ELEMS] == [("sgd", 4 * (8192 * 256 + 1) + 3), ("adamw", 4 * (8192 * 256 + 1) + 3)]
    assert {c[3] for c in upd} == set(fc.STEP_LAYOUTS) and {c[6] for c in cases if c[1] == "clip"} == set(fc.STEP_CLIPS)
    for e in ("sgd", "adamw"):
        mine = [c for c in upd if c[1] == e]
        assert {c[3] for c in mine} == set(fc.STEP_LAYOUTS) and {c[4] for c in mine} == set(fc.STEP_MIRRORS) and {c[5] for c in mine} == {0, 1}, e
        assert set(fc.STEP_NULLS) <= {x for c in mine + [c for c in upd if c[1] == "sgd_sched"] for x in c[7]}, e
    # the quad pre-test: all sixteen (start offset, end offset) pairs, each range with untouched quads on both sides
    r = fc.step_ranges("quad16", 4092)
    assert {(r0 % 4, r1 % 4) for r0, r1 in r} == {(a, b) for a in range(4) for b in range(4)} and len(r) == 16
    assert all(r[i][1] + 8 <= r[i + 1][0] for i in range(15))
    assert fc.step_ranges("inquad", 4098) == [(41, 43)] and fc.step_ranges("intail", 4103) == [(4101, 4103)] and fc.step_ranges("border", 4099) == [(4094, 4098)]
    assert len(fc.step_ranges("r32", 4100)) == 32 and fc.step_ranges("past", 4096) == [(4096, 4104), (4094, 4101)] and fc.step_selected("past", 4096) == [4094, 4095]
    assert fc.step_selected("empty", 4101) == [] and fc.step_selected("adjacent", 4094) == list(range(8, 22))
    assert fc.step_selected("intail", 5) == [4] and fc.step_selected("inquad", 4) == [1, 2]
    # the refusals the GPU test provokes
    assert fc.fill_step_args_refuses(False, False, True, 0, 0, False) and fc.fill_step_args_refuses(True, True, True, 0, 0, False)
    assert fc.fill_step_args_refuses(True, False, True, 0, 33, True) and fc.fill_step_args_refuses(True, False, True, 0, 32, True) is None
    assert fc.fill_step_args_refuses(True, True, False, 1, 0, False) and fc.fill_step_args_refuses(True, True, True, 2, 1, False)


def test_areas_sweep_covers_what_it_was_written_for():
    cases = fc.CASES["areas"]
    assert fc.areas_cases() == cases
    assert {c[1] for c in cases} == {1, 2, 19, 256} and {c[2] for c in cases} == {0, 1, 2} and {c[3] for c in cases if c[2] == 2} == {0, 1}
    assert {1, 4095, 4096, 4097, 1024 * 4096 + 1} == {c[4] for c in cases}
    assert any(0 <= c[5] < c[1] for c in cases) and any(c[5] >= c[1] for c in cases) and any(c[5] < 0 for c in cases)
    from tests import loss_step_reference as R
    for c in cases[:-1]:          # predictions and labels on both sides of [0, ncls), the ignore index among the labels
        pred, label = R.areas_inputs(c)
        assert c[4] < 64 or (pred.min() < 0 and pred.max() >= c[1] and (label.astype("int64") == c[5]).any() == (c[2] != 2 or 0 <= c[5] <= 255)), c[0]
        assert c[4] < 64 or c[2] == 2 and c[1] == 256 or label.astype("int64").max() >= c[1], c[0]


def test_restated_loss_and_step_grids_at_known_points():
    """computed by hand from csrc/loss_pixel.hpp, csrc/loss.hip, csrc/loss_ext/loss_ext.hip and csrc/optim.hip"""
    assert [fc.stream_grid(n, 1024) for n in (0, 1, 256, 257, 262144, 262145, 327680)] == [1, 1, 1, 2, 1024, 1024, 1024]
    assert fc.stream_grid(1048576, 4096) == 4096 and fc.loss_depth(1048576, 4096) == 1 and fc.loss_depth(1048577, 4096) == 2
    assert fc.stream_grid(32768, 128) == 128 and fc.loss_depth(32769, 128) == 2 and fc.loss_depth(5 * 256 * 256, 1024) == 2
    assert fc.shape_ok(1, 1, 1, 1) and not fc.shape_ok(1, 1, 1, 2 ** 31) and fc.shape_ok(1, 1, 1, 2 ** 31 - 1) and not fc.shape_ok(0, 1, 1, 1)
    assert [fc.lx_chunks(c) for c in (1, 8, 9, 16, 17, 64)] == [1, 1, 2, 2, 3, 8] and fc.lx_stride(6) == 27 and fc.lx_stride(17) == 75
    ohem = [c for c in fc.CASES["loss"] if c[1] == "ohem" and fc.loss_npix(c) == 36000][0]
    assert fc.loss_grids(ohem) == (141, 141, 128)
    assert [fc.clip_grid(n) for n in (1, 4099, 2097152, 2097159)] == [1, 4, 2048, 2048] and fc.clip_depth(2097152) == 4 and fc.clip_depth(2097159) == 9
    assert fc.clip_depth(3) == 1 and fc.clip_depth(4096) == 4
    assert [fc.step_grid(n) for n in (3, 4099, 8388608, 8388615)] == [1, 4, 8192, 8192] and fc.step_body_tail(4099) == (1024, 3) and fc.step_body_tail(3) == (0, 3)
    assert [fc.areas_grid(n) for n in (1, 4096, 4097, 1024 * 4096, 1024 * 4096 + 1)] == [1, 1, 2, 1024, 1024]


def test_loss_and_step_input_conditions_hold_in_float64():
    """what the exact comparisons of the GPU tests rest on, from the float64 references alone: no non-ignored pixel of an OHEM case other
    than the k-th (the tie and constant cases: other than its exact ties) within 1e-5 of the threshold; with range_mult = 0 every element
    outside the ranges of a step case moves by more than 4 ulp of itself"""
    from tests import loss_step_reference as R
    from tests.test_gpu_ohem import assert_input_margin, INF
    branches = set()
    for c in fc.CASES["loss"]:
        if c[1] != "ohem":
            continue
        x = R.loss_inputs(c)
        for z in (x["la"], x["lb"]):
            r = R.ohem_reference(c, z, x["labels"])
            assert_input_margin(r, tied_with_kth=r["tied"])
            nv = int(r["valid"].sum())
            branches.add("keep-all" if r["threshold"] == INF else "thresh" if r["threshold"] == c[13] else "k-th")
            if c[9] == "grid":
                pv = r["p"][r["valid"]]
                assert int((pv == r["threshold"]).sum()) >= 3 or r["threshold"] == c[13], c[0]
    assert branches == {"keep-all", "thresh", "k-th"}
    for c in fc.CASES["step"]:
        if c[1] != "clip":
            worst, outside = R.step_condition(c)
            assert worst > 1.0, "%s: an element outside the ranges moves by %.3g x 4 ulp" % (c[0], worst)
            assert outside == c[2] - len(fc.step_selected(c[3], c[2]))


def test_mha_sweep_covers_what_it_was_written_for():
    """every length of the list without dropout; dropout at p in {0.1, 0.5} on both sides of the LDS threshold of the VALU backward and at the
    lengths the sweep was asked to hold; ordinary inputs under dropout (no probability underflows there: kept == read back > 0)"""
    cases = fc.CASES["mha"]
    assert {c[3] for c in cases if c[5] == 0.0} == set(fc.MHA_LS)
    drop = [c for c in cases if c[5] > 0.0]
    assert {17, 33, 110, 111, 128} <= {c[3] for c in drop} and {c[5] for c in drop} == {0.1, 0.5}
    assert all(c[4] == "ordinary" for c in drop)
    assert fc.mha_cases() == cases


def test_msda_sweep_covers_what_it_was_written_for():
    """every kernel kind under every build that has it, twice (the regime list says which exist); every head count, batch size, dtype, input
    regime, layout and refmode; the written-out list is what msda_cases() returns"""
    cases = fc.CASES["msda"]
    assert fc.msda_cases() == cases and 55 <= len(cases) <= 80
    hits = dict(fc.regime_hits("msda"))
    for k in fc.MSDA_KINDS:
        for b in fc.MSDA_BUILDS:
            name = "%s, build (%d, %d)" % (k, b[0], b[1])
            if b[0] == 1 and k in ("FWD_BAND", "GRAD_BAND", "FINALIZE"):
                assert name not in hits and not any(fc._msda_has(k, b)(c) for c in cases)
            else:
                assert len(hits[name]) >= 2, name
    assert {c[2] for c in cases} == {1, 2, 3, 4, 8, 16} and {c[1] for c in cases} == {1, 2, 3}
    assert {c[8].partition("+")[0] for c in cases} == set(fc.MSDA_REFMODES) and {c[7] for c in cases} == set(fc.MSDA_LAYOUTS)
    assert all(c[2] == 8 for c in cases if c[8].endswith("+dref"))
    assert fc.msda_band_geometry(fc.MSDA_BAND4, 1, 8)[:2] == (4, 7) and fc.msda_band_geometry(fc.MSDA_BAND4, 1, 8, 3)[:2] == (4, 3)
    assert fc.msda_band_geometry(fc.MSDA_BAND2A, 1, 8)[0] == 2 and fc.msda_band_geometry(fc.MSDA_BAND2B, 1, 8)[0] == 2
    assert fc.msda_band_geometry(fc.MSDA_FIN3, 1, 8) == (0, 0, 0) and fc.msda_band_geometry(((64, 64),), 2, 8) == (0, 0, 0)


def test_gconv_sweep_covers_what_it_was_written_for():
    """one assertion per gap the sweep was written to close in csrc/gconv.hip, against the mirrored launch arithmetic"""
    cases = fc.CASES["gconv"]
    assert fc.gconv_cases() == cases and 40 <= len(cases) <= 50
    bwd = [c for c in cases if c[11] != "none"]
    dims = {c[0]: fc.gconv_dims(c) for c in cases}
    # output channels per group different from input channels per group, on both sides, Og = 4 and Og no power of two, forward and data gradient
    assert {4, 12, 20} <= {c[6] for c in bwd if c[6] != c[5] and fc._gc_has_dx(c)} and any(c[6] < c[5] for c in bwd) and any(c[6] > c[5] for c in bwd)
    # a second trip of each grid-stride loop: forward (cap 4096), data gradient (cap 4096), forward with statistics (cap ceil(2048 / nslices))
    loops = [c for c in cases if fc._gc_fwd_grid(c)[3]]
    assert any(not c[9].startswith("stats") and fc._gc_fwd_grid(c)[1] == 4096 for c in loops)
    assert any(fc._gc_has_dx(c) and fc.gconv_grid(dims[c[0]][5], dims[c[0]][0], False)[1:] == (4096, 1, True) for c in cases)
    assert any(c[9].startswith("stats") and fc._gc_fwd_grid(c)[1] == fc._ceil_div(2048, fc._gc_fwd_grid(c)[2]) and fc._gc_fwd_grid(c)[2] > 1 for c in loops)
    # dbias: in the full call and alone
    assert sum(c[11] == "all" for c in cases) >= 2 and sum(c[11] == "dbias" for c in cases) >= 2
    # block shapes that are no powers of two: idle threads at quads 3, 5, 6, 12 on either side; a ragged last channel slice on either side
    assert {3, 5, 6, 12} <= {fc._gc_fwd_quads(c) for c in cases} | {fc._gc_dgrad_quads(c) for c in cases}
    assert any(fc._gc_fwd_quads(c) > 64 and fc._gc_fwd_quads(c) % 64 for c in cases) and any((fc._gc_dgrad_quads(c) or 0) > 64 and fc._gc_dgrad_quads(c) % 64 for c in cases)
    # tiny and awkward maps: H or W of 1 and of 2, M below a tile, M % 4 != 0, even sizes under stride 2
    assert {1, 2} <= {v for c in cases for v in (c[2], c[3])}
    assert any(dims[c[0]][4] < fc._gc_fwd_tile(c) for c in cases) and any(dims[c[0]][4] % 4 for c in cases)
    assert any(c[7] == 2 and c[2] % 2 == 0 and c[3] % 2 == 0 for c in cases)
    # batch strides larger than the map, for each of in_bs, out_bs, dy_bs and dx_bs
    for i, need in enumerate((lambda c: True, lambda c: True, lambda c: c[11] != "none", fc._gc_has_dx)):
        assert sum("bs" in c[10][i] and need(c) for c in cases) >= 4, i
    # the weight gradient's slice plan: S = 1, slices no multiple of the unroll, S limited by the thread count, a ragged last thread block
    plans = [fc._gc_plan(c) for c in cases if fc._gc_plan(c) is not None]
    assert any(p[2] == 1 for p in plans) and any(p[2] > 1 and p[1] % 4 for p in plans) and any(p[0] % 256 for p in plans)
    assert any(fc._gc_plan(c) is not None and 1048576 // fc._gc_plan(c)[0] < dims[c[0]][4] // 32 for c in cases)
    # call forms: dw alone, dbias alone, dx alone; bias without scale; ReLU together with statistics; float16 at Cg other than 4
    assert {"dw", "dbias", "dx", "dx-acc+dw"} <= {c[11] for c in cases} and {"bias", "stats+bias", "stats+relu"} <= {c[9] for c in cases}
    assert {4, 8, 32} <= {c[5] for c in cases if c[8] == "f16"} and {"none", "bias", "fold+relu"} == {c[9] for c in cases if c[8] == "f16"}
    # C % 8 != 0 is inside the domain only as a slice of a wider buffer
    odd = [c for c in cases if dims[c[0]][0] % 8]
    assert odd and all("ld" in c[10][0] for c in odd)
    assert not fc.gconv_in_domain(odd[0][:10] + (("dense",) + odd[0][10][1:],) + odd[0][11:])


def _conv_point(N, H, W, C, OC, k, stride, pad, dtype, side, epilogue="none", arm=None, views="", knobs=()):
    """a case tuple for a dense layer, for the mirrored predicates alone"""
    return ("point", N, H, W, C, OC, k, stride, pad, 1, dtype, side, epilogue, arm or ("none" if side == "fwd" else "dx"), views, tuple(knobs), (), "ordinary", "", 0)


def test_conv_sweep_covers_what_it_was_written_for():
    """one assertion per gap the sweep was written to close in csrc/conv.hip / csrc/igemm8p.hpp, against the mirrored host-side decisions"""
    cases = fc.CASES["conv"]
    assert fc.conv_cases() == cases and 100 <= len(cases) <= 140
    single = [c for c in cases if c[11] in ("fwd", "bwd")]
    bwd = [c for c in single if c[11] == "bwd"]
    kind, copy, feats = fc._cv_kind, fc._cv_copy, fc.conv_feats
    assert {kind(c) for c in single} == set(fc.CONV_KINDS)
    # every kernel kind runs the masked / statistics epilogue and an addend (the thin kernel, which takes no addend: accumulate)
    for k in fc.CONV_KINDS:
        mine = [c for c in bwd if kind(c) == k]
        assert any({"mask", "stats"} <= feats(c) for c in mine), k
        assert any(("accumulate" if k == "thin" else "addend") in feats(c) for c in mine), k
    # the 256x256 LDS-DMA kernel and the parity-class kernel: stat_x and a strided mask; the 256x256 kernel with a strided addend too
    for k in ("8p", "s2"):
        mine = [c for c in bwd if kind(c) == k]
        assert any("stat_x" in feats(c) for c in mine) and any(fc._cv_view_kind(c, "mask") in fc.CONV_VIEWS for c in mine), k
        assert any(fc._cv_view_kind(c, "dx") in fc.CONV_VIEWS for c in mine), k
    assert any(kind(c) == "8p" and fc._cv_view_kind(c, "addend") in fc.CONV_VIEWS for c in bwd)
    # both epilogue copies of igemm_body with every feature of either side; the 8-phase copy with every feature
    for cp in ("vec", "scalar", "8p"):
        mine = [c for c in single if copy(c) == cp]
        assert set(fc._CV_FWD_FEATS) <= set().union(*[feats(c) for c in mine if c[11] == "fwd"]), cp
        assert set(fc._CV_BWD_FEATS) | {"mask_scale"} <= set().union(*[feats(c) for c in mine if c[11] == "bwd"]), cp
    # each tile, each in-block K split, the cross-block split, the pair kernel and the 256x256 kernel with a ragged M and a ragged OC tile
    for k in fc.CONV_KINDS:
        if k != "thin":
            assert any(kind(c) == k and fc._cv_ragged(c, 1) for c in single), k
            assert k == "s2" or any(kind(c) == k and fc._cv_ragged(c, 0) for c in single), k
    # 256x32 through the ladder: 24 channels on the vector epilogue, 6 and 7 on the scalar one, each with mask + statistics on the backward side
    for ch, cp in ((24, "vec"), (6, "scalar"), (7, "scalar")):
        assert any(c[4] == ch and kind(c) == "256x32" and copy(c) == cp and not c[15] and {"mask", "stats"} <= feats(c) for c in bwd), ch
        assert any(c[11] == "fwd" and c[5] == ch and kind(c) == "256x32" and copy(c) == cp for c in single), ch
    # the scalar epilogue by the channel count and, separately, by alignment alone, on the 64x64 and 128x128 tiles
    for k in ("64x64 G1", "128x128 G1"):
        assert any(kind(c) == k and copy(c) == "scalar" and fc.conv_gemm_dims(c)[1] % 8 for c in single), k
    assert any(kind(c).startswith("64x64") and fc._cv_off_grid_only(c) for c in single) and any(kind(c).startswith("128x128") and fc._cv_off_grid_only(c) for c in single)
    # the 256x256 kernel: C = 64, OC = 264, M = 330, k = 3 and k = 1 under both k orders, every backward epilogue of the issue, the forward's fp32 output
    p8 = [c for c in single if kind(c) == "8p"]
    assert all(fc.conv_gemm_dims(c) == (330, 264) and (c[5] if c[11] == "bwd" else c[4]) == 64 for c in p8)
    assert {(c[6], dict(c[15])["igemm8p_cmajor"]) for c in p8 if c[11] == "bwd"} == {(3, 0), (3, 1), (1, 0), (1, 1)}
    assert {"none", "stats", "mask", "mask+stats", "mask+stats+stat_x", "mask+scale", "addend", "addend+mask+stats+stat_x", "accumulate",
            "accumulate+mask+stats"} <= {c[12] for c in p8 if c[11] == "bwd"}
    assert any(c[11] == "fwd" and "out_f32" in feats(c) for c in p8)
    refused = [c for c in single if dict(c[15]).get("conv_tile") == 7 and kind(c) != "8p"]
    assert len(refused) == 1 and not fc.igemm8p_ok(fc.conv_problem(refused[0])[0]) and fc.conv_route(refused[0]) == ("64x64", 1, "scalar")
    # the cross-block split at 2, 3 and 8 copies asked, with mask + statistics + stat_x and with an addend; one case with fewer k-tiles than copies
    xk = [c for c in bwd if kind(c) == "xk"]
    assert {dict(c[15])["xk"] for c in xk} == {2, 3, 8} and any({"mask", "stats", "stat_x"} <= feats(c) for c in xk) and any("addend" in feats(c) for c in xk)
    assert any(fc.conv_k_tiles(fc.conv_problem(c)[0]) < dict(c[15])["xk"] for c in xk)
    # the parity-class kernel: the three tap lattices, both 256-pixel maps, both layer widths, every epilogue operand, each with its generic twin
    s2 = [c for c in bwd if kind(c) == "s2"]
    assert {(c[6], c[8]) for c in s2} == {(3, 1), (5, 2), (2, 0)} and {c[1:4] for c in s2} == {(1, 16, 16), (2, 8, 16)} and {c[5] for c in s2} == {64, 128}
    assert {"mask", "stats", "stat_x", "addend", "mask_scale", "accumulate"} <= set().union(*[feats(c) for c in s2])
    assert all(fc.conv_route(c, True)[:2] == ("64x64", 1) for c in s2)
    # the pair kernel: dw and dbias given, mask + statistics on the data-gradient half
    assert any(kind(c) == "pair" and c[13] == "dx+dw+dbias" and {"mask", "stats"} <= feats(c) for c in bwd)
    # the thin kernel: OC 6 and 7, C 32 / 64 / 256, MASK 0 / 1 / 2, with and without accumulate, each with the generic kernels as twin
    thin = [c for c in bwd if kind(c) == "thin"]
    assert {c[5] for c in thin} == {6, 7} and {c[4] for c in thin} == {32, 64, 256} and all(c[6] == 1 for c in thin)
    assert any("accumulate" in feats(c) for c in thin) and any("mask_is_x" in feats(c) for c in thin) and any("mask" in feats(c) and "mask_is_x" not in feats(c) for c in thin)
    assert all(fc.conv_route(c, True)[0] != "thin" for c in thin)
    # every view kind for every tensor role
    for side in ("fwd", "bwd"):
        for role in fc.CONV_ROLES[side]:
            assert {fc._cv_view_kind(c, role) for c in single} >= set(fc.CONV_VIEWS), role
    # the grouped entry points, one launch each, in every dtype they take
    assert {c[10] for c in cases if c[11] == "multi"} == {"bf16", "f32"} and {c[10] for c in cases if c[11] == "group"} == {"bf16", "f32", "f16"}
    assert all(fc.conv_group_is_one_launch(c) for c in cases if c[11] in ("multi", "group"))
    # mask draws need no margin, but forward ReLU cases do: they exist in every dtype
    assert {c[10] for c in single if c[11] == "fwd" and "relu" in feats(c)} == {"f32", "bf16", "f16"}


def test_mirrored_conv_plan_reproduces_the_recorded_table():
    """the mirrored bna_plan (and through it conv_plan, conv_is_vec, conv_k_tiles, conv_blocks, conv_takes_128, igemm8p_ok) against
    tests/golden/bna_supported.json: all 3780 rows under all nine knob sets, with no scratch registered (the cross-block split is unreachable,
    as in tests/test_conv_plan_cpu.py, whose sweep and knob sets these are)"""
    import json
    from tests import test_conv_plan_cpu as tp
    with open(tp.GOLDEN) as f:
        gold = json.load(f)
    rows = tp.rows()
    assert len(rows) == 3780 and len(tp.KNOB_SETS) == 9 and gold["knob_sets"] == [n for n, _ in tp.KNOB_SETS]
    for name, knobs in tp.KNOB_SETS:
        kn = dict(fc.CONV_KNOBS)
        kn.update(knobs)
        got = []
        for N, HW, C, OC, k, dt in rows:
            a, _ = fc.conv_problem(_conv_point(N, HW, HW, C, OC, k, 1, k // 2, ("f32", "bf16")[dt], "fwd", "bias+residual+relu+stats"), kn)
            got.append("1" if kn["no_bna"] != 1 and fc.bna_plan(a, kn, False)[0] != "none" else "0")
        diff = [(r, w, g) for r, w, g in zip(rows, gold["answers"][name], got) if w != g]
        assert not diff, "%s: %d rows differ from the recorded answers, first (N, HW, C, OC, k, dtype), recorded, mirrored: %s" % (name, len(diff), diff[:8])


def test_mirrored_predicates_at_known_points():
    """the shapes the fixed tests and the model use, whose path is known from the dispatchers' comments"""
    assert fc.bn_rowgeom(64) == (256, 16) and fc.bn_rowgeom(1024) == (256, 1) and fc.bn_rowgeom(2048) == (512, 1) and fc.bn_rowgeom(1028) == (257, 1)
    assert fc.bn_rowgeom(12) is None and fc.bn_rowgeom(2052) is None
    assert fc.gn_use_fused(256, 256, 32) and not fc.gn_use_fused(4097, 256, 32) and not fc.gn_use_fused(16, 1024, 2) and fc.gn_use_fused(1, 64, 4)
    assert fc.ln_bwd_blocks(10752, 256) == (168, False) and fc.ln_bwd_blocks(100000, 256) == (256, True) and fc.ln_bwd_blocks(633, 256, 0, 0, 256) == (20, False)
    assert [fc.vec_width(c, False) for c in (64, 20, 6)] == [8, 4, 1] and [fc.vec_width(c, True) for c in (64, 20, 6)] == [4, 4, 1]
    assert fc.vec_width(12, True, (8, 1)) == 1 and fc.vec_width(64, True, (8, 1)) == 8 and fc.vec_width(12, False, (4, 1)) == 4
    assert fc.pool_split(64, 64, 256, 1536, (1, 3, 6, 8)) and not fc.pool_split(16, 16, 256, 256, (1, 3, 6, 8)) and not fc.pool_split(64, 64, 100, 100, (1,))
    assert fc.pool_bwd_kernel(32, 32, 64, (1, 3, 6, 8)) == "table" and fc.pool_bwd_kernel(5, 32, 64, (8,)) == "gather" and fc.pool_bwd_kernel(32, 32, 6, (1,)) == "scalar"
    assert fc.pyramid_grouped(256, (1, 3, 6, 8), 32, 32, 2, True) and not fc.pyramid_grouped(256, (1, 3, 6, 8), 32, 32, 2, False)
    assert fc.pyramid_grouped(12, (5, 6), 26, 27, 4, True) and not fc.pyramid_grouped(12, (5, 6), 26, 27, 2, True)
    assert fc.resize_bwd_wide(256, 8, 8, 32, 32) and not fc.resize_bwd_wide(256, 8, 8, 31, 32) and not fc.resize_bwd_wide(6, 1, 1, 32, 32)
    assert fc.mha_bwd_stages_probs(110) and not fc.mha_bwd_stages_probs(111) and fc.mha_bwd_stages_probs(1) and not fc.mha_bwd_stages_probs(128)
    assert fc.mha_path(True, 110, 0, True) == 1 and fc.mha_path(False, 110, 0, True) == 0 and fc.mha_path(True, 1, 0, True) == 0
    assert fc.mha_path(True, 110, 1, True) == 0 and fc.mha_path(True, 110, 0, False) == 0 and fc.mha_path(True, 2, 0, True) == 1
    assert [fc.mha_tiles(L) for L in (1, 16, 17, 110, 113, 128)] == [1, 1, 2, 7, 8, 8]
    assert [fc.mha_fwd_chunks(L) for L in (1, 32, 33, 110, 128)] == [1, 1, 2, 4, 4]
    assert [fc.gconv_block(q) for q in (3, 8, 64, 80)] == [(3, 85), (8, 32), (64, 4), (64, 4)] and fc.gconv_grid(64, 320, False)[2] == 2
    assert fc.gconv_wgrad_plan(221, 32, 4) == (288, 37, 6) and fc.gconv_wgrad_plan(20, 32, 4)[2] == 1 and fc.gconv_wgrad_plan(4225, 2048, 4) == (18432, 76, 56)
    assert fc.gconv_grid(4225, 2048, True) == (265, 256, 8, True) and fc.gconv_grid(8 * 64 * 64, 256, True) == (2048, 2048, 1, False)
    assert fc.gconv_grid(257 * 257, 256, False) == (4129, 4096, 1, True) and fc.gconv_grid(257 * 257, 32, False) == (517, 517, 1, False)
    # csrc/conv.hip's own comments.  The cross-block split's table (igemm_xk_copies): 8x8x512 -> 512 3x3 at batch 8 is 64 tiles of 72 k-tiles
    # and takes four copies, 16x16x1024 -> 256 (128 tiles, 144 k-tiles) too, 16x16x256 -> 256 (128 tiles, 36 k-tiles) keeps the in-block
    # split; "9 k-tiles on 8 copies: per = 2 -> 5 copies"; fp32 and a context without scratch never split
    kn = dict(fc.CONV_KNOBS)
    xk = lambda *a_: fc.conv_problem(_conv_point(*a_), kn)[0]
    a = xk(8, 8, 8, 512, 512, 3, 1, 1, "bf16", "fwd")
    assert (fc.conv_blocks(a, 64, 64), fc.conv_k_tiles(a)) == (64, 72) and fc.igemm_xk_copies(a, kn, True) == 4 and fc.igemm_xk_copies(a, kn, False) == 0
    assert fc.conv_plan(a, kn, True) == ("xk", 4, False) and fc.conv_plan(a, kn, False) == ("64x64", 4, False)
    assert fc.igemm_xk_copies(xk(8, 16, 16, 1024, 256, 3, 1, 1, "bf16", "fwd"), kn, True) == 4 and fc.igemm_xk_copies(xk(8, 16, 16, 256, 256, 3, 1, 1, "bf16", "fwd"), kn, True) == 0
    assert fc.igemm_xk_copies(xk(8, 8, 8, 512, 512, 3, 1, 1, "f32", "fwd"), kn, True) == 0
    assert fc.igemm_xk_copies(xk(2, 9, 11, 64, 72, 3, 1, 1, "bf16", "fwd"), dict(kn, xk=8), True) == 5          # 9 k-tiles
    # the ladder: "the decoder's 32x32x1536 -> 512 3x3 forward" at batch 8 is exactly 256 blocks of 128x128 with 216 k-tiles: two wave groups;
    # "512 [blocks] at 64x64x256 -> 256": the plain 128x128 tile; a layer with at most 32 output channels: 256x32
    assert fc.conv_plan(xk(8, 32, 32, 1536, 512, 3, 1, 1, "bf16", "fwd"), kn, True) == ("128x128", 2, False)
    assert fc.conv_plan(xk(8, 32, 32, 1536, 512, 3, 1, 1, "bf16", "fwd"), dict(kn, no_ksplit128=1), True) == ("128x128", 1, False)
    assert fc.conv_plan(xk(8, 64, 64, 256, 256, 3, 1, 1, "bf16", "fwd"), kn, True) == ("128x128", 1, False)
    assert fc.conv_plan(xk(8, 64, 64, 256, 6, 1, 1, 0, "bf16", "fwd"), kn, True) == ("256x32", 1, False)
    # the 256x256 kernel from 160 blocks with at least 16 k-tiles of 64, or 96 blocks with 144: 128x128x256 -> 256 3x3 at batch 8 is 512 x 1 blocks
    big = xk(8, 128, 128, 256, 256, 3, 1, 1, "bf16", "fwd")
    assert fc.igemm8p_ok(big) and fc.conv_plan(big, kn, True) == ("8p", 1, False) and fc.conv_plan(big, dict(kn, igemm8p_min_blocks=0), True)[0] == "128x128"
    assert not fc.igemm8p_ok(xk(8, 128, 128, 96, 256, 3, 1, 1, "bf16", "fwd")) and not fc.igemm8p_ok(xk(8, 128, 128, 256, 256, 3, 1, 1, "f32", "fwd"))
    # the parity-class kernel (S2_CASES of tests/test_gpu_conv_fuzz.py): 3x3 stride 2 on 2 x 16 x 16 x 64; a 1x1 only under the knob -1; not at
    # 2 x 8 x 8 (128 input pixels: 32 rows per class), not with dilation, and not when the knob says 1
    s2 = lambda *a_, **kw: fc.igemm_s2_ok(fc.conv_problem(_conv_point(*a_), kn)[0], dict(kn, **kw))
    assert s2(2, 16, 16, 64, 64, 3, 2, 1, "bf16", "bwd") and s2(2, 16, 32, 64, 128, 5, 2, 2, "bf16", "bwd") and s2(2, 16, 16, 64, 128, 2, 2, 0, "f32", "bwd")
    assert not s2(8, 32, 32, 512, 1024, 1, 2, 0, "bf16", "bwd") and s2(8, 32, 32, 512, 1024, 1, 2, 0, "bf16", "bwd", no_s2_dgrad=-1)
    assert not s2(2, 8, 8, 64, 64, 3, 2, 1, "bf16", "bwd") and not s2(2, 16, 16, 64, 64, 3, 2, 1, "bf16", "bwd", no_s2_dgrad=1) and not s2(2, 16, 16, 64, 64, 3, 1, 1, "bf16", "bwd")
    # the thin backward: "8x128x128x256 -> 6 ... 4 channel chunks x 128 pixel chunks": 8 channels per thread, 32 pixel slots, 1024 pixels per block
    a, w = fc.conv_problem(_conv_point(8, 128, 128, 256, 6, 1, 1, 0, "bf16", "bwd", arm="dx+dw+dbias"), kn)
    assert fc.thin_bwd_ok(a, w) and fc.thin_bwd_geometry(a, w, kn) == (8, 32, 1024, 0) and w.C // 64 == 4
    assert not fc.thin_bwd_ok(*fc.conv_problem(_conv_point(8, 128, 128, 256, 6, 1, 1, 0, "bf16", "bwd", "addend", "dx+dw"), kn))
    assert not fc.thin_bwd_ok(*fc.conv_problem(_conv_point(8, 128, 128, 96, 6, 1, 1, 0, "bf16", "bwd", arm="dx+dw"), kn))          # C no power of two
    assert not fc.thin_bwd_ok(*fc.conv_problem(_conv_point(8, 128, 128, 256, 9, 1, 1, 0, "bf16", "bwd", arm="dx+dw"), kn))
    # the pair: "16x16 / 8x8 layers" pair, "from ~1000 dgrad tiles on" (pair_max 768) they do not, nor without dw, nor at OC <= 32
    pairs = lambda *a_, **kw: fc.conv_bwd_pairs(*fc.conv_problem(_conv_point(*a_, **kw), kn), kn)
    assert pairs(8, 16, 16, 256, 256, 3, 1, 1, "bf16", "bwd", arm="dx+dw") and pairs(8, 8, 8, 512, 512, 3, 1, 1, "bf16", "bwd", arm="dx+dw+dbias")
    assert not pairs(8, 64, 64, 128, 128, 3, 1, 1, "bf16", "bwd", arm="dx+dw") and not pairs(8, 16, 16, 256, 256, 3, 1, 1, "bf16", "bwd")
    assert not pairs(8, 16, 16, 24, 256, 3, 1, 1, "bf16", "bwd", arm="dx+dw")
    # the epilogue's vec_ok: OC % 8, and every operand's slice on the 16-byte grid
    vk = lambda views, oc=72, dt="bf16": fc.conv_epilogue_vec_ok(fc.conv_problem(_conv_point(2, 9, 11, oc, 64, 3, 1, 1, dt, "bwd", "addend+mask+stats+stat_x", views=views), kn)[0])
    assert vk("") and vk("mask:ld8 addend:bs statx:ld+bs16") and not vk("mask:ld4") and not vk("addend:ld4") and not vk("statx:ld4") and not vk("dx:ld4")
    assert vk("mask:ld4", dt="f32") and not vk("mask:ld2", dt="f32") and not vk("", oc=20)


def test_window_cases():
    im = fc.WINDOW_IMAGE
    a, b = fc.WINDOW_ORIGINS["grid"], fc.WINDOW_ORIGINS["odd"]
    assert len(a) == len(b) and 0 < fc.WINDOW_SPLIT < len(a)
    for chunk in (slice(0, fc.WINDOW_SPLIT), slice(fc.WINDOW_SPLIT, None)):          # the two accumulate calls
        assert fc.window_vec4(im["W"], im["cw"], a[chunk]) and not fc.window_vec4(im["W"], im["cw"], b[chunk])
        assert sum(p != q for p, q in zip(a[chunk], b[chunk])) == 1
    for org in (a, b):
        assert all(0 <= y and y + im["ch"] <= im["H"] and 0 <= x and x + im["cw"] <= im["W"] for y, x in org)
        cov = fc.window_cover(org, im["H"], im["W"], im["ch"], im["cw"])
        assert {0, 1, 2, 3, 4} <= {v for row in cov for v in row}
        assert all(row[x] == 0 for row in cov for x in range(20, im["W"])), "the strip x >= 20 is uncovered"


def test_the_docstring_table_is_current():
    for line in fc.regime_table().splitlines():
        assert line.rstrip() in fc.__doc__, "tests/fuzz_cases.py: the docstring's regime table is stale; regime_table() gives\n" + fc.regime_table()


def test_dropout_elementwise_case_sizes():
    """one second-trip case per kernel above MAX_ELEMS, at 8192 x 256 + 1 lanes (2048 x 256 + 1 for the copy kernel); everything else small"""
    big = [c for c in fc.CASES["dropout"] if fc.drop_n(c) > fc.MAX_ELEMS]
    assert [fc.drop_n(c) for c in big] == [fc.DROP_LONG_MAX_ELEMS] and fc.DROP_LONG_MAX_ELEMS == fc.STEP_LONG_MAX_ELEMS - 3
    assert {fc.drop_n(c) for c in fc.CASES["dropout"] if c[1] == "element"} == {4, 1020, 1024, 1028, fc.DROP_LONG_MAX_ELEMS}
    assert {c[3] for c in fc.CASES["dropout"]} == set(fc.DROP_PS)
    from tests import dropout_reference as dr
    for c in fc.CASES["dropout"]:          # a channel-mode case that drops at all has planes of both kinds (a wrong plane index cannot hide)
        if c[1] == "channel" and c[3] >= 0.1:
            planes = dr.channel_mask(c[8], c[6], c[3], fc.drop_n(c), c[2][1], c[2][2]).reshape(c[2][0], c[2][1], c[2][2])[:, 0]
            assert 0 < int(planes.sum()) < planes.size, c[0]
    for c in fc.CASES["layernorm_drop"]:
        assert c[1] * c[2] * c[3] <= fc.MAX_ELEMS and c[1] * c[2] <= 700
    assert {c[3] for c in fc.CASES["layernorm_drop"]} == set(fc.LND_CS)
    for c in fc.CASES["conv_drop"]:
        assert c[1] * max(c[3], c[5]) <= fc.MAX_ELEMS and c[2] * c[4] <= fc.MAX_ELEMS
    assert ({c[1] for c in fc.CASES["conv_drop"]}, {c[2] for c in fc.CASES["conv_drop"]}, {c[4] for c in fc.CASES["conv_drop"]}) == (
        set(fc.CDROP_MS), set(fc.CDROP_CS), set(fc.CDROP_OCS))
    # a case emrt_conv2d_drop would refuse is no case: an output row that is not whole 16-byte chunks, in either type
    assert fc.conv_drop_vec_ok(64, 64, 64, 72, 76, 4) and not fc.conv_drop_vec_ok(64, 64, 64, 72, 74, 4) and not fc.conv_drop_vec_ok(64, 64, 64, 72, 76, 2) and not fc.conv_drop_vec_ok(63, 8, 12, 8, 8, 2)
    assert not fc.cdrop_in_domain(fc.CASES["conv_drop"][0][:5] + (12,) + fc.CASES["conv_drop"][0][6:])
    trips = {}
    for c in fc.CASES["elementwise"]:
        lanes, bytes_ = fc.ew_lanes(c), {"f32": 4, "bf16": 2, "f16": 2}[c[2]]
        if fc.ew_second_trip(c):
            assert c[1] not in trips and lanes == (2048 * 256 + 1 if c[1] == "memcpy" else fc.EW_TRIP), c
            trips[c[1]] = lanes
        else:
            assert lanes * 4 <= fc.MAX_ELEMS, c
    assert sorted(trips) == sorted(fc.EW_KERNELS) and fc.EW_LONG_MAX_ELEMS == fc.DROP_LONG_MAX_ELEMS


def test_attention_dropout_cases_leave_nothing_out_of_the_mask_comparison():
    """tests/test_gpu_mha_fuzz.py compares the device's kept / dropped pattern with the host model except where the float64 reference probability
    is below 1e-30.  Every dropout case runs all three paths (bf16 as dispatched: the MFMA kernels, staging or re-deriving the probabilities by
    mha_bwd_split; mha_valu = 1 and fp32: the VALU kernels on either side of mha_bwd_stages_probs), so: each side of each threshold has a dropout
    case that leaves out nothing, and no case leaves out more than half."""
    import torch
    from tests import mha_reference as mr
    shares = {}
    for c in fc.CASES["mha"]:
        if c[5] > 0:
            for d in mr.DTYPES:
                q, k = mr.make_inputs(c[4], c[1], c[2], c[3], c[7], d)[:2]
                shares[(c[0], d)] = float((torch.softmax(mr.scores(q, k), -1) < 1e-30).double().mean())
    assert len(shares) == 32 and max(shares.values()) <= 0.5
    for d in mr.DTYPES:
        for staged in (True, False):
            assert any(shares[(c[0], d)] == 0.0 for c in fc.CASES["mha"] if c[5] > 0 and fc.mha_bwd_stages_probs(c[3]) == staged), (d, staged)
    assert max(shares.values()) == 0.0          # today: nothing is left out in any dropout case
