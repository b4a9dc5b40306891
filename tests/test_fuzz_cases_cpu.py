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
