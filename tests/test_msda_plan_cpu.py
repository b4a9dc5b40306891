"""CPU: the deformable-attention planner, seen through emrt_msda_plan and emrt_msda_bwd_workspace_bytes.

emrt_msda_plan launches nothing -- it runs the planner emrt_msda_fwd / emrt_msda_bwd launch from and answers, per launch the call would
make and in launch order, (kernel kind, grid, threads, dynamic LDS bytes) -- so it works without a GPU.  A table of its answers over the
shapes and knob sets below pins every rung of the dispatcher (which first-stage kernel, chunk / band counts, whether max |dout| is scanned
separately, which scatter, its ranges and query split, the finalize count) and the workspace size: tests/golden/msda_plan.json, recorded
from the library BEFORE the host side of msda.hip was refactored into one plan (that library had no such query: its launches were logged
by a throw-away patch that recorded each launch site's kernel, grid, block and LDS bytes instead of launching).

Re-record (only when the dispatcher is changed on purpose):  python tests/test_msda_plan_cpu.py --record
"""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "msda_plan.json")

# EMRT_MSDA_K_* of include/emrt_hip.h, by value
KINDS = ["FWD_GLOBAL", "FWD_LDS", "FWD_BAND", "GRAD_GLOBAL", "GRAD_LDS", "GRAD_BAND", "ABSMAX", "SCATTER_MF", "SCATTER_LDS", "FINALIZE"]
F32, BF16, F16 = 0, 1, 2
CFG2, CFG3 = [(32, 32), (16, 16), (8, 8)], [(64, 64), (32, 32), (16, 16)]


def _row(name, B, shapes, Lq=None, M=8, P=6, dtype=BF16, dref=False):
    return dict(name=name, B=B, shapes=[list(hw) for hw in shapes], Lq=Lq or sum(h * w for h, w in shapes), M=M, P=P, dtype=dtype, dref=dref)


ROWS = (
    [_row("cfg2 B%d %s" % (B, n), B, CFG2, dtype=dt) for B in (8, 16) for n, dt in (("bf16", BF16), ("fp16", F16), ("fp32", F32))]
    + [_row("cfg3 B4 %s" % n, 4, CFG3, dtype=dt) for n, dt in (("bf16", BF16), ("fp16", F16), ("fp32", F32))]
    + [_row("decoder Lq110", 8, CFG2, Lq=110), _row("decoder Lq110 dref", 8, CFG2, Lq=110, dref=True),
       _row("decoder Lq110 dref fp32", 8, CFG2, Lq=110, dref=True, dtype=F32),
       _row("tiny Lq10", 1, [(2, 2), (2, 2), (1, 2)], Lq=10),
       _row("16|8|4 B1", 1, [(16, 16), (8, 8), (4, 4)]), _row("48|16|8 B1", 1, [(48, 48), (16, 16), (8, 8)]),
       _row("band-nonsquare B2", 2, [(64, 80), (32, 40), (16, 20)]), _row("band-nonsquare B2 fp16", 2, [(64, 80), (32, 40), (16, 20)], dtype=F16),
       _row("odd height 63x64 B1", 1, [(63, 64), (32, 32), (16, 16)]),           # no band plan exists
       _row("wide rows 4x400 B1", 1, [(4, 400), (2, 200), (1, 100)]),            # backward refused: a row does not fit a scatter slab
       _row("L4P4 B2", 2, [(32, 32), (16, 16), (8, 8), (4, 4)], P=4), _row("L3P4 B2", 2, CFG2, P=4), _row("L1P4 B2", 2, [(32, 32)], P=4),
       _row("L1P4 64x64 B2", 2, [(64, 64)], P=4),                                # one level too large for a slab: never the band kernel
       _row("L2P4 B2 unsupported", 2, [(32, 32), (16, 16)], P=4),
       _row("M4 Lq2048", 2, CFG2, Lq=2048, M=4), _row("M4 Lq2048 fp32", 2, CFG2, Lq=2048, M=4, dtype=F32),
       _row("M16 Lq2048", 1, CFG2, Lq=2048, M=16)]                              # 256 % (M * 4) == 0 but M > 8: no max |dout| scan, no query split
)

KNOB_DEFAULTS = dict(msda_fwd_global=0, msda_bwd_global=0, msda_bwd_dref_lds=1, msda_scatter_mfma=1, msda_scatter_qsplit=0, msda_scatter_cuts=0,
                     msda_fwd_chunks=0, msda_band_halo=0, msda_mf_bands=0, msda_lds_min_pairs=2048)
KNOB_SETS = [("default", {})] + [("%s=%d" % kv, dict([kv])) for kv in (
    ("msda_fwd_global", 1), ("msda_bwd_global", 1), ("msda_bwd_dref_lds", 0), ("msda_scatter_mfma", 0), ("msda_scatter_mfma", 2),
    ("msda_scatter_qsplit", -1), ("msda_scatter_qsplit", 2), ("msda_scatter_cuts", 3), ("msda_fwd_chunks", 2), ("msda_band_halo", 4),
    ("msda_mf_bands", 256), ("msda_lds_min_pairs", 1 << 30))]

# recorded by hand from the library before the refactoring: "kind grid | threads | LDS bytes" per launch, workspace bytes
ANCHORS = {
    "cfg2 B8 bf16": ("FWD_LDS 256,1,1 | 1024 | 90368", "GRAD_LDS 256,1,1 | 1024 | 90368; SCATTER_MF 64,4,1 | 512 | 152832", 6212096),
    "cfg2 B8 fp32": ("FWD_GLOBAL 1344,1,1 | 256 | 0", "GRAD_GLOBAL 1344,1,1 | 256 | 0; ABSMAX 168,1,1 | 256 | 0; SCATTER_LDS 64,4,1 | 1024 | 97040", 6212096),
    "cfg3 B4 bf16": ("FWD_BAND 256,1,1 | 1024 | 153600", "GRAD_BAND 256,1,1 | 1024 | 153600; SCATTER_LDS 32,16,1 | 1024 | 147728; FINALIZE 32,3,8 | 256 | 0",
                     30225152),
    "48|16|8 B1": ("FWD_BAND 64,1,1 | 1024 | 90112", "GRAD_BAND 64,1,1 | 1024 | 90112; SCATTER_LDS 8,16,1 | 1024 | 97040; FINALIZE 8,3,8 | 256 | 0", 2629696),
    "odd height 63x64 B1": ("FWD_GLOBAL 664,1,1 | 256 | 0",
                            "GRAD_GLOBAL 664,1,1 | 256 | 0; ABSMAX 83,1,1 | 256 | 0; SCATTER_LDS 8,16,1 | 1024 | 147728; FINALIZE 8,3,8 | 256 | 0", None),
}


def _show(rec):
    return None if rec is None else "; ".join("%s %d,%d,%d | %d | %d" % tuple(launch) for launch in rec)


def ask(L, row):
    """{"fwd": launches | None (refused), "bwd": ..., "ws": bytes}; bwd and ws for the training dtypes only.  A launch is [kind, gx, gy, gz, threads, LDS bytes]."""
    nl = len(row["shapes"])
    arr = (ctypes.c_int * (2 * nl))(*[v for hw in row["shapes"] for v in hw])
    shapes = ctypes.cast(arr, ctypes.c_void_p)
    out = (ctypes.c_int * 64)()

    def plan(backward):
        n = L.query("emrt_msda_plan", backward, row["B"], row["Lq"], row["M"], nl, row["P"], shapes, int(row["dref"]), row["dtype"], ctypes.cast(out, ctypes.c_void_p), 64)
        if n < 0:
            assert n == -1 and L.last_error().startswith("emrt_msda_plan: "), (n, L.last_error())
            return None
        assert n % 6 == 0 and 6 <= n <= 24
        return [[KINDS[out[i]]] + [out[i + k] for k in range(1, 6)] for i in range(0, n, 6)]

    ans = {"fwd": plan(0)}
    if row["dtype"] != F16:
        ans["bwd"] = plan(1)
        ans["ws"] = L.query("emrt_msda_bwd_workspace_bytes", row["B"], row["Lq"], row["M"], nl, row["P"], shapes, row["dtype"])
    return ans


def table(L, ask=ask):
    """{knob set: {row name: ask(row)}}"""
    out = {}
    for name, knobs in KNOB_SETS:
        want = dict(KNOB_DEFAULTS)
        want.update(knobs)
        old = [(k, L.set_tuning(k, v)) for k, v in want.items()]
        try:
            out[name] = {row["name"]: ask(L, row) for row in ROWS}
        finally:
            for k, v in old:
                L.set_tuning(k, v)
    return out


def _lib():
    from emrt_amd import _lib, build_ext
    build_ext.build(verbose=False)
    return _lib.lib()


def _gold():
    with open(GOLDEN) as f:
        return json.load(f)


def test_kind_names_are_the_headers():
    text = open(os.path.join(ROOT, "include", "emrt_hip.h")).read()
    assert [(n, int(v)) for n, v in re.findall(r"#define EMRT_MSDA_K_(\w+) (\d+)", text)] == [(n, i) for i, n in enumerate(KINDS)]


def test_the_recorded_table_is_not_trivial():
    gold = _gold()
    assert gold["rows"] == ROWS and gold["knob_sets"] == [n for n, _ in KNOB_SETS]
    assert len({r["name"] for r in ROWS}) == len(ROWS)
    d = gold["answers"]["default"]
    assert set(d) == {r["name"] for r in ROWS}
    seen = {launch[0] for a in d.values() for rec in (a["fwd"], a.get("bwd")) if rec for launch in rec}
    assert seen == set(KINDS), "kernel kinds no row reaches under default knobs: %s" % sorted(set(KINDS) - seen)
    refused = sorted(n for n, a in d.items() if a["fwd"] is None or ("bwd" in a and a["bwd"] is None))
    assert len(refused) >= 2, refused
    for r in ROWS:
        assert ("bwd" in d[r["name"]]) == ("ws" in d[r["name"]]) == (r["dtype"] != F16)
    for name, (fwd, bwd, ws) in ANCHORS.items():
        assert _show(d[name]["fwd"]) == fwd and _show(d[name]["bwd"]) == bwd, name
        assert ws is None or d[name]["ws"] == ws, name
    # every knob set moves at least one answer (a knob the planner stopped reading would pass unnoticed otherwise)
    for name, _ in KNOB_SETS[1:]:
        assert gold["answers"][name] != d, name


def test_plan_matches_the_recorded_table():
    gold = _gold()["answers"]
    got = table(_lib())
    for name, _ in KNOB_SETS:
        diff = [(r["name"], k, gold[name][r["name"]].get(k), got[name][r["name"]].get(k)) for r in ROWS for k in ("fwd", "bwd", "ws")
                if gold[name][r["name"]].get(k) != got[name][r["name"]].get(k)]
        assert not diff, "%s: %d answers differ from the recorded ones, first (row, which, recorded, got): %s" % (name, len(diff), diff[:4])


def test_plan_refuses_what_the_entry_points_refuse():
    L = _lib()
    arr = (ctypes.c_int * 6)(*[v for hw in CFG2 for v in hw])
    shapes, out = ctypes.cast(arr, ctypes.c_void_p), (ctypes.c_int * 24)()
    outp = ctypes.cast(out, ctypes.c_void_p)
    for args, why in (((0, 8, 1344, 8, 3, 6, shapes, 0, 3, outp, 24), "dtype"), ((1, 8, 1344, 8, 3, 6, shapes, 0, F16, outp, 24), "dtype"),
                      ((1, 8, 110, 4, 3, 6, shapes, 1, BF16, outp, 24), "M == 8"), ((0, 8, 1344, 8, 3, 5, shapes, 0, BF16, outp, 24), "(3,6), (4,4), (3,4), (1,4)"),
                      ((0, 8, 1344, 8, 5, 6, shapes, 0, BF16, outp, 24), "bad M/L/P"), ((0, 8, 1344, 8, 3, 6, None, 0, BF16, outp, 24), "level shapes"),
                      ((1, 8, 1344, 8, 3, 6, shapes, 0, BF16, outp, 6), "6 ints per launch")):
        assert L.query("emrt_msda_plan", *args) == -1 and why in L.last_error(), (args[:6], L.last_error())


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_msda_plan_cpu.py --record")
    sys.path.insert(0, ROOT)
    answers = table(_lib())
    with open(GOLDEN, "w") as f:
        json.dump({"rows": ROWS, "knob_sets": [n for n, _ in KNOB_SETS], "answers": answers}, f, indent=0)
        f.write("\n")
    for row in ROWS:
        a = answers["default"][row["name"]]
        print("%-26s fwd %s\n%26s bwd %s  ws %s" % (row["name"], _show(a["fwd"]), "", _show(a.get("bwd")), a.get("ws")))
