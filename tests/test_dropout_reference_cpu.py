"""tests/dropout_reference.py, held to csrc/drop_hash.hpp and to its own statistics.  No GPU.

Model = text: a stand-alone host program (its own main, generated into tmp_path) includes csrc/drop_hash.hpp, prints every function's words
for a table of (seed, salt, index, p), and the numpy model has to give the same words bit for bit.  The program is host code with its own
main, so it also runs once under the address and undefined-behaviour sanitizers, in the inherited environment.

The model's statistics: keep rates, independence inside a group, between neighbouring groups and between two salts, all within 5 standard
errors of the binomial at 2^22 groups.  Everything is deterministic (fixed seeds, salts and counts); the worst of all the comparisons below
is 4.2 standard errors.  The device is never held to statistics: the GPU sweeps hold it to this model exactly.
"""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from tests import dropout_reference as dr
from tests.test_abi_cpu import _host_cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "emrt_amd", "csrc")

SEEDS = (0, 1, 0x0123456789abcdef, dr.context_seed(), (1 << 64) - 1)
SALTS = (0, 1, 5, 1000, 0xFFFFFFFF)
INDEXES = (0, 1, 2, 3, 255, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 40) + 123, (1 << 63) + 7)
PS = (0.0, 2.0 ** -17, 0.1, 0.5, 0.999)
TABLE = list(itertools.product(SEEDS, SALTS, INDEXES, PS))

PROGRAM = r"""
#include "drop_hash.hpp"
#include <stdio.h>
#include <string.h>
struct Row { unsigned long long seed; unsigned salt; unsigned long long idx; float p; };
static const Row rows[] = {
%s
};
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, sizeof u); return u; }
int main() {
  for (const Row& r : rows) {
    uint32_t q[2], w[4], a[2];
    emrt::drop_quad(r.seed, r.salt, r.idx, q);
    emrt::drop_words8(r.seed, r.salt, (uint32_t)r.idx, w);
    emrt::mha_drop4(r.seed, r.salt, (unsigned)r.idx, a);
    const uint32_t thr = emrt::drop_thr16(r.p);
    const float u = emrt::uniform01(r.seed, r.salt, r.idx);
    unsigned kq = 0, kw = 0, ka = 0;
    for (int e = 0; e < 4; ++e) kq |= (unsigned)emrt::drop_quad_keep(q, e, thr) << e;
    for (int e = 0; e < 8; ++e) kw |= (unsigned)emrt::drop_keep8(w, e, thr) << e;
    for (int e = 0; e < 4; ++e) ka |= (unsigned)emrt::mha_keep4(a, e, thr) << e;
    printf("%%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%08x %%x %%x %%x %%x\n", emrt::mix32((uint32_t)r.idx), bits(u), q[0], q[1], w[0], w[1],
           w[2], w[3], a[0], a[1], thr, kq, kw, ka, (unsigned)(u >= r.p));
  }
  return 0;
}
"""


def _model_rows():
    seed = np.array([r[0] for r in TABLE], dtype=np.uint64)
    salt = np.array([r[1] for r in TABLE], dtype=np.uint64)
    idx = np.array([r[2] for r in TABLE], dtype=np.uint64)
    ps = [r[3] for r in TABLE]
    thr = np.array([dr.drop_thr16(p) for p in ps], dtype=np.uint32)
    u = dr.uniform01(seed, salt, idx)
    q, w, a = dr.drop_quad(seed, salt, idx), dr.drop_words8(seed, salt, idx), dr.mha_drop4(seed, salt, idx)

    def keeps(words, n):
        k = np.zeros(len(TABLE), dtype=np.uint32)
        for e in range(n):
            k |= (dr.lane16(words, np.full(len(TABLE), e)) >= thr).astype(np.uint32) << np.uint32(e)
        return k

    ge = u >= np.array(ps, dtype=np.float32)
    cols = [dr.mix32(idx), u.view(np.uint32), q[0], q[1], w[0], w[1], w[2], w[3], a[0], a[1], thr, keeps(q, 4), keeps(w, 8), keeps(a, 4), ge.astype(np.uint32)]
    return [tuple(int(c[i]) for c in cols) for i in range(len(TABLE))]


def _build(tmp_path, name, flags):
    src = tmp_path / (name + ".cpp")
    rows = ",\n".join("  {0x%xull, 0x%xu, 0x%xull, %sf}" % (s, t, i, float(np.float32(p)).hex()) for s, t, i, p in TABLE)
    src.write_text(PROGRAM % rows)
    exe = tmp_path / name
    r = subprocess.run([_host_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", HEADER_DIR] + flags + [str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, "exit %d\n%s" % (r.returncode, (r.stdout[-500:] + r.stderr[-3000:]))
    return r


def _parse(out):
    return [tuple(int(x, 16) for x in line.split()) for line in out.strip().splitlines()]


def test_the_header_includes_nothing_from_hip():
    text = open(os.path.join(HEADER_DIR, "drop_hash.hpp")).read()
    incs = [ln.strip() for ln in text.splitlines() if ln.strip().startswith("#include")]
    assert incs == ["#include <stdint.h>"], incs
    for fn in ("mix32", "uniform01", "drop_quad", "drop_quad_keep", "drop_thr16", "drop_words8", "drop_keep8", "mha_drop4", "mha_keep4"):
        assert "EMRT_DROP_FN" in [ln for ln in text.splitlines() if (" %s(" % fn) in ln and "{" in ln][0], fn
    for other in ("common.hpp", "attn.hip"):
        body = open(os.path.join(HEADER_DIR, other)).read()
        assert '#include "drop_hash.hpp"' in body and "uint32_t mix32(" not in body and "void mha_drop4(" not in body, other


def test_the_model_is_the_header_bit_for_bit(tmp_path):
    """every function of csrc/drop_hash.hpp, compiled by the host compiler, against the numpy model on every table row: index >= 2^32,
    salt 0, seed 0, the context's default seed word, and thresholds at p in {0, 2^-17, 0.1, 0.5, 0.999}"""
    assert any(i >= 1 << 32 for i in INDEXES) and 0 in SALTS and 0 in SEEDS and set(PS) == {0.0, 2.0 ** -17, 0.1, 0.5, 0.999}
    got = _parse(_run(_build(tmp_path, "drop_table", [])).stdout)
    want = _model_rows()
    assert len(got) == len(want) == len(TABLE)
    for row, g, w in zip(TABLE, got, want):
        assert g == w, "(seed, salt, index, p) = %r: header %r, model %r" % (row, g, w)
    # the thresholds the table is there for: p = 2^-17 truncates to 0 (nothing dropped), p = 0.999 to 65470
    assert [int(dr.drop_thr16(p)) for p in PS] == [0, 0, 6553, 32768, 65470]


def test_the_header_runs_clean_under_the_sanitizers(tmp_path):
    """the same program with -fsanitize=address,undefined (host code with its own main, the sanitizer runtime linked in: the test preloads nothing and runs it in the environment it inherits); same words, no report"""
    exe = _build(tmp_path, "drop_table_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = _run(exe)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    assert _parse(r.stdout) == _model_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# the model's statistics
# ---------------------------------------------------------------------------------------------------------------------------------
NGROUPS = 1 << 22
STAT_PS = (0.1, 0.3, 0.5)
STAT_SEEDS = (0x0123456789abcdef, 7, 0)
STAT_SALTS = (5, 6, 1000)
SALT_PAIRS = ((5, 6), (11, 12), (7, 8), (1, 2))
GATE = 5.0
WORST = {}          # test name -> the worst |observed - expected| / standard error it saw (printed with -s)


def _z(count, n, prob):
    return abs(count / n - prob) / math.sqrt(prob * (1.0 - prob) / n)


def _gate(name, what, count, n, prob):
    z = _z(count, n, prob)
    WORST[name] = max(WORST.get(name, 0.0), z)
    assert z <= GATE, "%s: %s: %d of %d, expected rate %.6f: %.2f standard errors" % (name, what, count, n, prob, z)


def _group_stats(name, lanes, thr, q, what):
    """lanes [positions][NGROUPS] uint32 16-bit uniforms; q the keep probability"""
    keep = [ln >= thr for ln in lanes]
    for e, k in enumerate(keep):
        _gate(name, "%s position %d keep rate" % (what, e), int(k.sum()), k.size, q)
        _gate(name, "%s position %d with the next group's" % (what, e), int((k[:-1] & k[1:]).sum()), k.size - 1, q * q)
    for e, f in itertools.combinations(range(len(keep)), 2):
        _gate(name, "%s positions %d and %d joint keep" % (what, e, f), int((keep[e] & keep[f]).sum()), keep[e].size, q * q)


def _lanes(words):
    return [(words[e >> 1] >> np.uint32(16 * (e & 1))) & np.uint32(0xFFFF) for e in range(2 * len(words))]


@pytest.mark.parametrize("fn,npos", [("drop_quad", 4), ("drop_words8", 8)])
def test_group_draws_keep_rate_and_independence(fn, npos):
    groups = np.arange(NGROUPS, dtype=np.uint64)
    for seed, salt in itertools.product(STAT_SEEDS, STAT_SALTS):
        lanes = _lanes(getattr(dr, fn)(seed, salt, groups))
        assert len(lanes) == npos
        for p in STAT_PS:
            _group_stats(fn, lanes, dr.drop_thr16(p), 1.0 - dr.p_eff(p), "%s seed %#x salt %d p %.1f" % (fn, seed, salt, p))
    print("%s: worst %.2f standard errors" % (fn, WORST[fn]))


@pytest.mark.parametrize("fn", ["drop_quad", "drop_words8"])
def test_group_draws_differ_between_two_salts(fn):
    """the same position at two salts of one step (the context's default seed): agreement (1 - p)^2 + p^2"""
    groups, name = np.arange(NGROUPS, dtype=np.uint64), fn + " salts"
    for s0, s1 in SALT_PAIRS:
        a, b = _lanes(getattr(dr, fn)(dr.context_seed(), s0, groups)), _lanes(getattr(dr, fn)(dr.context_seed(), s1, groups))
        for p in STAT_PS:
            thr, pe = dr.drop_thr16(p), dr.p_eff(p)
            for e in range(len(a)):
                agree = int(((a[e] >= thr) == (b[e] >= thr)).sum())
                _gate(name, "%s salts (%d, %d) p %.1f position %d agreement" % (fn, s0, s1, p, e), agree, NGROUPS, (1 - pe) ** 2 + pe ** 2)
    print("%s: worst %.2f standard errors" % (name, WORST[name]))


def test_uniform01_keep_rate_and_independence():
    idx, name = np.arange(NGROUPS, dtype=np.uint64), "uniform01"
    for p in STAT_PS:
        pe = math.ceil(float(np.float32(p)) * 16777216.0) / 16777216.0          # u = k 2^-24 >= p  <=>  k >= ceil(p 2^24)
        for seed, salt in itertools.product(STAT_SEEDS, STAT_SALTS):
            k = dr.uniform01(seed, salt, idx) >= np.float32(p)
            what = "uniform01 seed %#x salt %d p %.1f" % (seed, salt, p)
            _gate(name, what + " keep rate", int(k.sum()), k.size, 1 - pe)
            _gate(name, what + " with the next index", int((k[:-1] & k[1:]).sum()), k.size - 1, (1 - pe) ** 2)
        for s0, s1 in SALT_PAIRS:
            a, b = dr.uniform01(dr.context_seed(), s0, idx) >= np.float32(p), dr.uniform01(dr.context_seed(), s1, idx) >= np.float32(p)
            _gate(name, "uniform01 salts (%d, %d) p %.1f agreement" % (s0, s1, p), int((a == b).sum()), NGROUPS, (1 - pe) ** 2 + pe ** 2)
    print("%s: worst %.2f standard errors" % (name, WORST[name]))


def test_site_masks_are_the_documented_indexes():
    """the per-site functions against the index expressions written out element by element (small shapes)"""
    seed, salt, p = dr.context_seed(), 9, 0.5
    thr = dr.drop_thr16(p)
    m = dr.layernorm_mask(seed, salt, p, 3, 12)
    for row, c in ((0, 0), (1, 5), (2, 11)):
        h = dr.drop_quad(seed, salt, np.uint64((row * 12 + c) >> 2))
        assert m[row, c] == bool(((int(h[(c & 3) >> 1]) >> (16 * (c & 1))) & 0xFFFF) >= thr)
    assert np.array_equal(m.reshape(-1), dr.element_mask(seed, salt, p, 36))
    cm = dr.conv_drop_mask(seed, salt, p, 5, 24)
    for mm, n in ((0, 0), (3, 9), (4, 23)):
        h = dr.drop_words8(seed, salt, (mm * 24 + (n & ~7)) >> 3)
        assert cm[mm, n] == bool(((int(h[(n & 7) >> 1]) >> (16 * (n & 1))) & 0xFFFF) >= thr)
    ch = dr.channel_mask(seed, salt, p, 2 * 3 * 8, 3, 8).reshape(2, 3, 8)
    assert (ch == ch[:, :1]).all() and not np.array_equal(ch[0], ch[1])
    for n, c in ((0, 0), (1, 7)):
        assert ch[n, 2, c] == bool(dr.uniform01(seed, salt, np.uint64(n * 8 + c)) >= np.float32(p))
    B, M, L = 2, 3, 5
    a, v = dr.mha_mfma_mask(seed, salt, p, B, M, L), dr.mha_valu_mask(seed, salt, p, B, M, L)
    for b, h_, i, j in ((0, 0, 0, 0), (1, 2, 4, 3), (1, 0, 2, 4)):
        w = dr.mha_drop4(seed, salt, (((b * M + h_) * L + i) * 32 + (j >> 2)) & 0xFFFFFFFF)
        assert a[b, h_, i, j] == bool(((int(w[(j & 3) >> 1]) >> (16 * (j & 1))) & 0xFFFF) >= thr)
        assert v[b, h_, i, j] == bool(dr.uniform01(seed, salt, np.uint64(((b * M + h_) * L + i) * L + j)) >= np.float32(p))
