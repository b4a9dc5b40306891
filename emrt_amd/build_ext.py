"""Builds emrt_amd/csrc/libemrt_hip.so and, beside it, emrt_amd/csrc/libemrt_hip_augment.so (csrc/augment_ext/*.hip: the entry points of
include/emrt_hip_augment.h, kept out of the first library because its ABI is frozen) and emrt_amd/csrc/libemrt_hip_sampler.so
(csrc/sampler_ext/*.hip: include/emrt_hip_sampler.h, for the same reason) with hipcc for gfx950, in-tree.  GROUPS is the table of the three;
EXTRA_GROUPS holds the library added next, emrt_amd/csrc/libemrt_hip_loss.so (csrc/loss_ext/*.hip: include/emrt_hip_loss.h), and MORE_GROUPS the
ones after it: emrt_amd/csrc/libemrt_hip_tta.so (csrc/tta_ext/*.hip: include/emrt_hip_tta.h).  all_groups() is those five rows, pinned by the tests
of the fifth library; LATER_GROUPS holds what came after them, emrt_amd/csrc/libemrt_hip_mstta.so (csrc/mstta_ext/*.hip:
include/emrt_hip_mstta.h), and every_group() is every row: what build(), _headers() and source_digest() walk.

What is rebuilt is decided by CONTENT: every object and the library carry a `<file>.inputs` stamp with the sha256 of the sources, headers,
compiler path and flags they were built from; "reused" therefore means "built from exactly these inputs", on whatever machine.

hipcc cross-compiles without a GPU, so this runs in the build container as the "does it build" check."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libemrt_hip.so")
SOURCES = ["conv.hip", "norm.hip", "msda.hip", "attn.hip", "spatial.hip", "loss.hip", "optim.hip", "elementwise.hip", "gconv.hip", "augment.hip", "scene.hip"]
HEADER = os.path.join(os.path.dirname(HERE), "include", "emrt_hip.h")      # the public C-ABI: csrc/common.hpp includes it, so it is an input of every object
AUG_DIR = os.path.join(CSRC, "augment_ext")
AUG_LIB = os.path.join(CSRC, "libemrt_hip_augment.so")
AUG_SOURCES = ["augment_ext.hip"]
AUG_HEADER = os.path.join(os.path.dirname(HERE), "include", "emrt_hip_augment.h")      # includes emrt_hip.h; the sources include csrc/augment_map.hpp
SMP_DIR = os.path.join(CSRC, "sampler_ext")
SMP_LIB = os.path.join(CSRC, "libemrt_hip_sampler.so")
SMP_SOURCES = ["sampler_ext.hip"]
SMP_HEADER = os.path.join(os.path.dirname(HERE), "include", "emrt_hip_sampler.h")      # includes emrt_hip.h; the sources include csrc/philox.hpp
# one row per library: (library, the directory of its sources and objects, sources, public header)
GROUPS = [(LIB, CSRC, SOURCES, HEADER), (AUG_LIB, AUG_DIR, AUG_SOURCES, AUG_HEADER), (SMP_LIB, SMP_DIR, SMP_SOURCES, SMP_HEADER)]
LOSS_DIR = os.path.join(CSRC, "loss_ext")
LOSS_LIB = os.path.join(CSRC, "libemrt_hip_loss.so")
LOSS_SOURCES = ["loss_ext.hip"]
LOSS_HEADER = os.path.join(os.path.dirname(HERE), "include", "emrt_hip_loss.h")      # the sources include csrc/common.hpp and csrc/loss_pixel.hpp
# the rows behind the first three, same form and same rules (GROUPS itself stays the table of the three libraries the sampler's tests pin)
EXTRA_GROUPS = [(LOSS_LIB, LOSS_DIR, LOSS_SOURCES, LOSS_HEADER)]
TTA_DIR = os.path.join(CSRC, "tta_ext")
TTA_LIB = os.path.join(CSRC, "libemrt_hip_tta.so")
TTA_SOURCES = ["tta_ext.hip"]
TTA_HEADER = os.path.join(os.path.dirname(HERE), "include", "emrt_hip_tta.h")      # the sources include csrc/common.hpp and csrc/scene_norm.hpp
# the rows behind those (EXTRA_GROUPS is pinned at one row by the loss library's tests, as GROUPS is at three)
MORE_GROUPS = [(TTA_LIB, TTA_DIR, TTA_SOURCES, TTA_HEADER)]
MST_DIR = os.path.join(CSRC, "mstta_ext")
MST_LIB = os.path.join(CSRC, "libemrt_hip_mstta.so")
MST_SOURCES = ["mstta_ext.hip"]
MST_HEADER = os.path.join(os.path.dirname(HERE), "include", "emrt_hip_mstta.h")      # the sources include csrc/common.hpp and csrc/scene_norm.hpp
# the rows behind all_groups() (MORE_GROUPS is pinned at one row and all_groups() at the three tables above by the tta library's tests)
LATER_GROUPS = [(MST_LIB, MST_DIR, MST_SOURCES, MST_HEADER)]
# (the include path is relative to csrc/, where hipcc runs: the flags are hashed, and an absolute path would tie the digest to one checkout)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-result", "-I../../include"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _digest(paths, extra=()):
    """sha256 over the CONTENT of the given files (in the given order) and the extra strings (compiler, flags)."""
    import hashlib
    h = hashlib.sha256()
    for e in extra:
        h.update(str(e).encode() + b"\0")
    for p in paths:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()


def _stamp(target):
    return target + ".inputs"


def _fresh(target, digest):
    """The object / library exists and was built from exactly these inputs (content hash recorded beside it): modification times are not
    trusted -- the built files travel between machines (gpurun snapshots, the driver's boxes) where they mean nothing."""
    try:
        with open(_stamp(target)) as f:
            return os.path.exists(target) and f.read().strip() == digest
    except OSError:
        return False


def all_groups():
    """Every library's row: GROUPS, then EXTRA_GROUPS, then MORE_GROUPS."""
    return GROUPS + EXTRA_GROUPS + MORE_GROUPS


def every_group():
    """Every library's row: all_groups(), then LATER_GROUPS."""
    return all_groups() + LATER_GROUPS


def _headers():
    """csrc/*.hpp and the public headers: inputs of every object of every library."""
    return [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".hpp")] + [g[3] for g in every_group()]


def source_digest():
    """Content hash of everything the libraries are built from: the sources of every row of every_group(), csrc/*.hpp, include/*.h, the compiler
    path and the flags."""
    return _digest([os.path.join(d, s) for _, d, sources, _ in every_group() for s in sources] + _headers(), [_hipcc()] + FLAGS)


LAST_BUILD = {"mode": None, "digest": None, "compiled": [], "linked": []}      # what the last build() call did: "compiled" | "linked" | "reused"


def build(force=False, verbose=True):
    """Builds every library of every_group(); -> the path of libemrt_hip.so (the others are AUG_LIB, SMP_LIB, LOSS_LIB, TTA_LIB and MST_LIB).  Only the objects whose inputs
    changed are compiled, and only the libraries that hold one of them are linked again."""
    hipcc = _hipcc()
    hdrs = _headers()
    objs, jobs = {g[0]: [] for g in every_group()}, []
    for lib, d, sources, _ in every_group():
        for src in sources:
            s = os.path.join(d, src)
            o = os.path.join(d, src.replace(".hip", ".o"))
            objs[lib].append(o)
            dg = _digest([s] + hdrs, [hipcc] + FLAGS)
            if force or not _fresh(o, dg):
                jobs.append(([hipcc] + FLAGS + ["-c", s, "-o", o], o, dg, lib))

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr[-4000:]))

    def compile_one(job):
        cmd, o, d, _ = job
        if os.path.exists(_stamp(o)):
            os.remove(_stamp(o))
        run(cmd)
        with open(_stamp(o), "w") as f:
            f.write(d + "\n")
        return cmd[-3]

    LAST_BUILD["compiled"] = []
    for lib in {j[3] for j in jobs}:      # a library whose objects are about to change loses its stamp first: a stamp beside a library
        if os.path.exists(_stamp(lib)):   # therefore says "linked after the last compile of any of its objects", even after an interrupted build
            os.remove(_stamp(lib))
    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            for done in ex.map(compile_one, jobs):
                LAST_BUILD["compiled"].append(os.path.basename(done))
                if verbose:
                    print("[emrt_amd.build] compiled", os.path.basename(done), flush=True)
    total = source_digest()
    linked = LAST_BUILD["linked"] = []
    for lib, _, _, _ in every_group():
        if force or any(j[3] == lib for j in jobs) or not (os.path.exists(lib) and os.path.exists(_stamp(lib))):
            if os.path.exists(_stamp(lib)):
                os.remove(_stamp(lib))
            run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs[lib] + ["-o", lib])
            with open(_stamp(lib), "w") as f:
                f.write(total + "\n")
            linked.append(os.path.basename(lib))
            if verbose:
                print("[emrt_amd.build] linked", lib, flush=True)
        elif not _fresh(lib, total):      # its own objects are all as they were (another library's source changed): the same library, the new digest
            with open(_stamp(lib), "w") as f:
                f.write(total + "\n")
    LAST_BUILD["mode"] = ("compiled" if jobs else "linked") if linked else "reused"
    LAST_BUILD["digest"] = total
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
