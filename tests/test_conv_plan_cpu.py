"""CPU: the convolution dispatcher's tile plan, seen through emrt_conv2d_bna_supported.

That entry point launches nothing -- it runs the operand-transform eligibility test and the tile ladder on the host and answers 0 / 1 -- so
it works without a GPU ("device pointers" are an aligned constant that is never read, the stream is null).  Its answer is 1 exactly when the
ladder ends on a 64x64 tile (the cross-block K split needs registered scratch and is not reached here), so a table of its answers over a sweep
of layer shapes and knob sets pins the order and the thresholds of the ladder's rungs: tests/golden/bna_supported.json, recorded from the
library BEFORE the host side of conv.hip was refactored into one tile plan.

Re-record (only when the ladder is changed on purpose):  python tests/test_conv_plan_cpu.py --record
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bna_supported.json")

SWEEP = dict(N=[1, 4, 8], HW=[8, 16, 32, 64, 128], C=[32, 64, 96, 128, 192, 256, 512, 1024, 2048], OC=[16, 32, 64, 128, 256, 512, 2048],
             k=[1, 3], dtype=[0, 1])
KNOB_SETS = [("default", {}), ("no_bna=-1", {"no_bna": -1}), ("no_bna=1", {"no_bna": 1})] + [("conv_tile=%d" % t, {"conv_tile": t}) for t in (1, 3, 5, 6, 7, 8)]


def rows():
    """The sweep in its recorded order: (N, HW, C, OC, k, dtype), dtype fastest."""
    return [(N, HW, C, OC, k, dt) for N in SWEEP["N"] for HW in SWEEP["HW"] for C in SWEEP["C"] for OC in SWEEP["OC"] for k in SWEEP["k"]
            for dt in SWEEP["dtype"]]


def ask(L, N, HW, C, OC, k, dtype):
    """emrt_conv2d_bna_supported for a dense stride-1 "same" k x k layer (the argument list of emrt_conv2d_bna)."""
    p = ctypes.c_void_p(0x10000)          # "a device pointer": aligned, never read
    H = W = HW
    return L.query("emrt_conv2d_bna_supported", p, p, p, p, p, N, H, W, C, C, H * W * C, H, W, OC, OC, H * W * OC, OC, H * W * OC, k, k, 1, k // 2,
                   1, 0, p, 1, p, float(N * H * W), 1e-5, 0.9, p, p, p, p, p, p, 1, p, dtype, None)


def table(L):
    """{knob set: "0110..."}: one character per row of rows()."""
    out = {}
    for name, knobs in KNOB_SETS:
        want = dict(no_bna=0, conv_tile=0)          # the knobs the sets touch, at their defaults unless the set says otherwise
        want.update(knobs)
        old = [(k, L.set_tuning(k, v)) for k, v in want.items()]
        try:
            out[name] = "".join(str(ask(L, *r)) for r in rows())
        finally:
            for k, v in old:
                L.set_tuning(k, v)
    return out


def _lib():
    from emrt_amd import _lib, build_ext
    build_ext.build(verbose=False)
    return _lib.lib()


def test_bna_supported_matches_the_recorded_table():
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["sweep"] == SWEEP and gold["knob_sets"] == [n for n, _ in KNOB_SETS]
    n = len(rows())
    assert n == 3780
    # the table cannot pass by being all one value: under default knobs each answer covers at least a quarter of the rows
    ones = gold["answers"]["default"].count("1")
    assert n // 4 <= ones <= n - n // 4, ones
    got = table(_lib())
    for name, _ in KNOB_SETS:
        want = gold["answers"][name]
        assert len(want) == n and set(want) <= {"0", "1"}
        diff = [(r, int(w), int(g)) for r, w, g in zip(rows(), want, got[name]) if w != g]
        assert not diff, "%s: %d rows differ from the recorded answers, first (N, HW, C, OC, k, dtype), recorded, got: %s" % (name, len(diff), diff[:8])


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_conv_plan_cpu.py --record")
    sys.path.insert(0, ROOT)
    answers = table(_lib())
    with open(GOLDEN, "w") as f:
        json.dump({"sweep": SWEEP, "knob_sets": [n for n, _ in KNOB_SETS], "answers": answers}, f, indent=0)
        f.write("\n")
    for name, _ in KNOB_SETS:
        print("%-12s %4d of %d rows answer 1" % (name, answers[name].count("1"), len(answers[name])))
