"""CPU: tests/msda_reference.py against the oracle's torch expression of the operation, the sweep's cases (tests/fuzz_cases.py, op "msda")
against the planner, and the calibration of MSDA_BOUND -- floors recomputed over the sweep's own cases, every mutant beyond twice its bound
in the regime built for it, and the distance of every sample coordinate from an integer line.  No GPU: emrt_msda_plan launches nothing."""
import ctypes

import pytest
import torch

from tests import fuzz_cases as fc
from tests import msda_reference as ms

F64 = torch.float64
CASES = fc.CASES["msda"]
DT = {"f32": 0, "bf16": 1, "f16": 2}
KNOB_DEFAULTS = dict(msda_fwd_global=0, msda_bwd_global=0, msda_bwd_dref_lds=1, msda_scatter_mfma=1, msda_scatter_qsplit=0, msda_scatter_cuts=0,
                     msda_fwd_chunks=0, msda_band_halo=0, msda_mf_bands=0, msda_lds_min_pairs=2048)


def _ids(cases):
    return [c[0] for c in cases]


# ---- the reference against the oracle ---------------------------------------------------------------------------------------------------
def _oracle(value, offw, ref, shapes, M, P):
    """the oracle's core function (grid_sample) on float64 leaves"""
    from oracle.emrt_torch import deformable_attention_core_func
    B, Lq = offw.shape[:2]
    L = len(shapes)
    tp = M * L * P
    off = offw[..., :2 * tp].reshape(B, Lq, M, L, P, 2)
    aw = torch.softmax(offw[..., 2 * tp:3 * tp].reshape(B, Lq, M, L * P), -1).reshape(B, Lq, M, L, P)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=F64).reshape(1, 1, 1, L, 1, 2)
    rl = ref.expand(B, Lq, ref.shape[2], 2)
    if rl.shape[2] == 1:
        rl = rl.expand(B, Lq, L, 2)
    loc = rl.reshape(B, Lq, 1, L, 1, 2) + off / norm
    return deformable_attention_core_func(value.reshape(B, -1, M, 32), shapes, loc, aw)


SMALL = [("small-%dx%d-%s-%s" % (len(sh), P, refmode, regime), B, M, sh, Lq, P, regime, "dense", refmode, {}, ("f32", (), ()), 7000 + i)
         for i, (B, M, sh, Lq, P, refmode, regime) in enumerate(
             (B, M, sh, Lq, P, refmode, regime)
             for sh, P in ((fc.MSDA_ODD3, 6), (fc.MSDA_ODD4, 4), (fc.MSDA_MF3, 4), (((7, 10),), 4))
             for (B, M, Lq, refmode, regime) in ((2, 2, 23, "shared-1", "ordinary"), (2, 3, None, "batch-1", "border"),
                                                 (3, 1, 17, "shared-L", "far"), (2, 2, 9, "batch-L", "lastquery")))]


@pytest.mark.parametrize("case", SMALL, ids=_ids(SMALL))
def test_reference_matches_the_oracle(case):
    """out and every gradient to 1e-9, every build and every refmode (the centres regime sits on the kinks of the bilinear weights, where
    autograd's one-sided choice is grid_sample's own: excluded)"""
    _, B, M, shapes, Lq, P, regime, _, refmode, _, _, _ = case
    inp = ms.make_inputs(case, "f32")
    mine = ms.exact(inp, shapes, M, P)
    v, o, r = (inp[k].clone().requires_grad_(True) for k in ("value", "offw", "ref"))
    out = _oracle(v, o, r, shapes, M, P)
    out.backward(inp["dout"].reshape(out.shape))
    Lv = v.shape[1]
    L = len(shapes)
    tp = M * L * P
    assert (out.detach().reshape(B, -1, M, 32) - mine["out"]).abs().max().item() < 1e-9
    assert (v.grad.reshape(B, Lv, M, 32) - mine["dvalue"]).abs().max().item() < 1e-9
    assert (o.grad[..., :2 * tp].reshape(mine["doff"].shape) - mine["doff"]).abs().max().item() < 1e-9
    assert (o.grad[..., 2 * tp:].reshape(mine["dlogit"].shape) - mine["dlogit"]).abs().max().item() < 1e-9
    assert (r.grad - ms.reduce_dref(mine["dref"], refmode.startswith("shared"))).abs().max().item() < 1e-9
    mag = ms.magnitude(inp, shapes, M, P)
    for k in ("out", "dvalue", "doff", "dlogit", "dref"):          # a magnitude bounds its value, entry by entry
        assert bool((mag[k] + 1e-12 >= mine[k].abs()).all()), k


# ---- the cases against the planner ----------------------------------------------------------------------------------------------------
def _lib():
    from emrt_amd import _lib, build_ext
    build_ext.build(verbose=False)
    return _lib.lib()


def plan_kinds(L_, case, backward, knobs=None):
    """the kernel kinds emrt_msda_plan answers for the case under its knobs (every other knob at its default), and the launches"""
    _, B, M, shapes, _, P, _, _, refmode, case_knobs, expect, _ = case
    want = dict(KNOB_DEFAULTS)
    want.update(case_knobs)
    want.update(knobs or {})
    old = [(k, L_.set_tuning(k, v)) for k, v in want.items()]
    try:
        nl = len(shapes)
        arr = (ctypes.c_int * (2 * nl))(*[v for hw in shapes for v in hw])
        out = (ctypes.c_int * 64)()
        n = L_.query("emrt_msda_plan", int(backward), B, fc.msda_lq(case), M, nl, P, ctypes.cast(arr, ctypes.c_void_p), int(refmode.endswith("+dref")),
                     DT[expect[0]], ctypes.cast(out, ctypes.c_void_p), 64)
        assert n > 0, L_.last_error()
        return tuple(fc.MSDA_KINDS[out[i]] for i in range(0, n, 6)), [[out[i + j] for j in range(6)] for i in range(0, n, 6)]
    finally:
        for k, v in reversed(old):
            L_.set_tuning(k, v)


def test_the_planner_answers_expect_for_every_case():
    from tests.test_msda_plan_cpu import KINDS, KNOB_DEFAULTS as PLAN_DEFAULTS
    assert tuple(KINDS) == fc.MSDA_KINDS and PLAN_DEFAULTS == KNOB_DEFAULTS and set(fc.MSDA_KNOBS) <= set(KNOB_DEFAULTS)
    L_ = _lib()
    for case in CASES:
        dtype, fwd, bwd = case[10]
        got, launches = plan_kinds(L_, case, False)
        assert got == fwd, (case[0], "forward", got, fwd)
        NB, halo, slab = fc.msda_band_geometry(case[3], case[1], case[2], case[9].get("msda_band_halo", 0))
        if "FWD_BAND" in fwd:          # the mirrored band geometry is the planner's: blocks = B M NB, and the slab bytes follow from (NB, halo)
            assert NB and launches[0][1] == case[1] * case[2] * NB and launches[0][5] == slab, (case[0], NB, halo, slab, launches)
        if bwd is not None:
            got, _ = plan_kinds(L_, case, True)
            assert got == bwd, (case[0], "backward", got, bwd)
        if dtype == "bf16":            # what the GPU sweep relies on: the matrix-product scatter has a plan for every bf16 case, the integer one always
            assert "SCATTER_MF" in plan_kinds(L_, case, True, {"msda_scatter_mfma": 2})[0], case[0]
            assert "SCATTER_LDS" in plan_kinds(L_, case, True, {"msda_scatter_mfma": 0})[0], case[0]


# ---- floors, bounds, the distance guarantee -------------------------------------------------------------------------------------------
def _floors(case):
    """{(tensor key): worst per-row error of the best a correct kernel can do} and the case's distance from the integer lines"""
    _, B, M, shapes, _, P, regime, _, refmode, _, expect, _ = case
    dtype = expect[0]
    inp = ms.make_inputs(case, dtype)
    rec = {"line": ms.line_distance(inp["offw"], inp["ref"], shapes, M, P) if regime != "centres" else float("inf")}
    want, mag = ms.exact(inp, shapes, M, P), ms.magnitude(inp, shapes, M, P)
    shared = refmode.startswith("shared")
    if dtype in ("bf16", "f16"):
        rec["out"] = ms.row_errors(ms.contract_16(inp, shapes, M, P, dtype), want["out"], mag["out"]).max().item()
    if dtype == "bf16":
        for kind in ("lds", "mf"):
            got = ms.contract_bwd(inp, shapes, M, P, dtype, kind)
            e = ms.worst_errors(got, want, mag, inp, M, dtype, kind, shared)
            rec[("dvalue", ms.dvalue_key(regime, kind))] = e["dvalue"]
            rec["doff"], rec["dlogit"] = e["doff"], e["dlogit"]
    if dtype == "f32" or refmode.endswith("+dref"):
        ch = ms.evaluate_f32(inp, shapes, M, P)
        e = ms.worst_errors({k: ch[k] for k in ("out", "doff", "dlogit", "dref")}, want, mag, inp, M, dtype, "lds", shared)
        if refmode.endswith("+dref"):
            rec["dref"] = e["dref"]
        if dtype == "f32":
            rec["out"], rec["doff"], rec["dlogit"] = e["out"], e["doff"], e["dlogit"]
            got = {"dvalue": ms.scatter_lds(ch, inp, M, "f32")}
            rec[("dvalue", ms.dvalue_key(regime, "lds"))] = ms.worst_errors(got, want, mag, inp, M, dtype, "lds")["dvalue"]
    return rec


@pytest.fixture(scope="module")
def floors():
    return {c[0]: _floors(c) for c in CASES}


def test_every_coordinate_keeps_its_distance_from_the_integer_lines(floors):
    for c in CASES:
        assert floors[c[0]]["line"] >= ms.NEAR_LINE, (c[0], floors[c[0]]["line"])


def test_floors_and_bounds(floors):
    worst = {}
    for c in CASES:
        dtype = c[10][0]
        for k, v in floors[c[0]].items():
            if k != "line":
                key = (dtype,) + (k if isinstance(k, tuple) else (k,))
                if v > worst.get(key, (-1.0, None))[0]:
                    worst[key] = (v, c[0])
    for key in sorted(worst):
        print("floor %-34s %.3e  (%s)" % (" ".join(key), worst[key][0], worst[key][1]))
    for key, (v, cid) in worst.items():
        dtype, tensor = key[0], key[1]
        bound = ms.MSDA_BOUND[dtype][tensor] if tensor != "dvalue" else ms.MSDA_BOUND[dtype]["dvalue"][key[2]]
        margin = ms.DREF_MARGIN if tensor == "dref" else ms.FLOOR_MARGIN[dtype]
        assert v <= bound / margin, "%s: floor %.3e (%s) above bound %.3e / %g" % (key, v, cid, bound, margin)
    # every key of the table is calibrated by some case
    keys = {(d, t) + ((k,) if t == "dvalue" else ()) for d, tb in ms.MSDA_BOUND.items() for t, b in tb.items() for k in (b if t == "dvalue" else (None,))}
    assert keys == set(worst), keys ^ set(worst)


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
def _mutant_excess(case, mutant, tensors, kind="lds"):
    """{tensor: worst error of the mutant / bound} over `tensors`"""
    _, B, M, shapes, _, P, regime, _, refmode, knobs, expect, _ = case
    dtype = expect[0]
    inp = ms.make_inputs(case, dtype)
    want, mag = ms.exact(inp, shapes, M, P), ms.magnitude(inp, shapes, M, P)
    got = mutant(inp, shapes, M, P)
    got = {k: got[k] for k in tensors}
    e = ms.worst_errors(got, want, mag, inp, M, dtype, kind, refmode.startswith("shared"))
    return {k: e[k] / ms.bound_of(dtype, k, regime, kind) for k in tensors}


def _of(regime, cond=lambda c: True):
    return [c for c in CASES if c[6] == regime and cond(c)]


BAND_EDGE = _of("bandedge", lambda c: c[10][0] == "bf16")
LAST = _of("lastquery", lambda c: c[10][0] != "f16")
BORDER = _of("border")
PER_LEVEL = [c for c in CASES if c[8].partition("+")[0].endswith("L") and c[6] in ("ordinary", "border", "lastquery") and len(c[3]) > 1]
SPIKE = _of("spike")


@pytest.mark.parametrize("case", BAND_EDGE, ids=_ids(BAND_EDGE))
def test_mutant_band_block_drops_what_it_has_not_staged(case):
    NB, halo, _ = fc.msda_band_geometry(case[3], case[1], case[2], case[9].get("msda_band_halo", 0))
    x = _mutant_excess(case, lambda i, s, M, P: ms.drop_outside_band(i, s, M, P, NB, halo), ("out", "doff", "dlogit", "dvalue"))
    assert min(x.values()) > 2.0, x


@pytest.mark.parametrize("case", LAST, ids=_ids(LAST))
def test_mutant_last_query_added_twice(case):
    dref = case[8].endswith("+dref")
    for kind in ("lds", "mf") if case[10][0] == "bf16" else ("lds",):
        x = _mutant_excess(case, ms.last_query_twice, ("dvalue", "dref") if dref else ("dvalue",), kind)
        assert min(x.values()) > 2.0, (kind, x)


@pytest.mark.parametrize("case", PER_LEVEL, ids=_ids(PER_LEVEL))
def test_mutant_every_level_reads_level_0s_point(case):
    tensors = ("out",) if case[10][0] == "f16" else ("out", "doff", "dlogit", "dvalue")
    x = _mutant_excess(case, ms.ref_level0, tensors)
    assert min(x.values()) > 2.0, x


@pytest.mark.parametrize("case", BORDER, ids=_ids(BORDER))
def test_mutant_partly_outside_samples_dropped_whole(case):
    tensors = ("out",) if case[10][0] == "f16" else ("out", "doff", "dlogit", "dvalue")
    x = _mutant_excess(case, ms.drop_partly_outside, tensors)
    assert min(x.values()) > 2.0, x


@pytest.mark.parametrize("case", SPIKE, ids=_ids(SPIKE))
def test_mutant_scale_taken_without_the_spike_rows(case):
    dtype = case[10][0]
    x = _mutant_excess(case, lambda i, s, M, P: {"dvalue": ms.scale_without_spikes(i, s, M, P, dtype)}, ("dvalue",))
    assert x["dvalue"] > 2.0, x


def test_the_mutant_regimes_are_not_empty():
    assert len(BAND_EDGE) >= 2 and len(LAST) >= 2 and len(BORDER) >= 2 and len(PER_LEVEL) >= 2 and len(SPIKE) >= 2
    assert any(c[8].endswith("+dref") for c in LAST)
