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
