"""Builds emrt_amd/csrc/libemrt_hip.so and the libraries beside it with hipcc for gfx950, in-tree.  LIBRARIES is the one table of them, in
build order: a row per library with its short name, its path, the directory of its sources and objects, the sources and the public header
under include/ (each side library is a library of its own because the ABI of the headers before it is frozen).  LATER_LIBRARIES and OPEN_LIBRARIES
continue it (below: why there are three lists, and which one a new library joins).  library(name) looks a row up in all of them.

What is rebuilt is decided by CONTENT: every object and the library carry a `<file>.inputs` stamp with the sha256 of the sources, headers,
compiler path and flags they were built from; "reused" therefore means "built from exactly these inputs", on whatever machine.

hipcc cross-compiles without a GPU, so this runs in the build container as the "does it build" check."""
import os
import subprocess
import sys
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libemrt_hip.so")
SOURCES = ["conv.hip", "norm.hip", "msda.hip", "attn.hip", "spatial.hip", "loss.hip", "optim.hip", "elementwise.hip", "gconv.hip", "augment.hip", "scene.hip"]
HEADER = os.path.join(os.path.dirname(HERE), "include", "emrt_hip.h")      # the public C-ABI: csrc/common.hpp includes it, so it is an input of every object
Library = namedtuple("Library", "name lib dir sources header")


def _side(name):
    """The row of a side library: csrc/<name>_ext/<name>_ext.hip -> csrc/libemrt_hip_<name>.so, declared in include/emrt_hip_<name>.h"""
    return Library(name, os.path.join(CSRC, "libemrt_hip_%s.so" % name), os.path.join(CSRC, name + "_ext"), [name + "_ext.hip"],
                   os.path.join(os.path.dirname(HERE), "include", "emrt_hip_%s.h" % name))


# what build(), _headers() and source_digest() walk, in this order (the digest depends on it)
LIBRARIES = [Library("main", LIB, CSRC, SOURCES, HEADER)] + [_side(n) for n in ("augment", "sampler", "loss", "tta", "mstta")]
# The libraries that arrived after the suite pinned the table above to its six rows (tests/test_abi_cpu.py): same row type, built, hashed and looked
# up with the others, after them.  The two lists become one in the first change that may edit that test.
LATER_LIBRARIES = [_side("rot")]
# That list is pinned to its one row too (tests/test_rot90_cpu.py).  This one is the open end: its test asks that a row is in it and behaves like the
# others, never that the rows are its whole content, so the next library is one more row here and no fourth list.
OPEN_LIBRARIES = [_side("bnd")]


def all_libraries():
    """LIBRARIES + LATER_LIBRARIES + OPEN_LIBRARIES: every library build() makes, in build order."""
    return LIBRARIES + LATER_LIBRARIES + OPEN_LIBRARIES


def library(name):
    """The row of LIBRARIES, LATER_LIBRARIES or OPEN_LIBRARIES with that short name."""
    for row in all_libraries():
        if row.name == name:
            return row
    raise KeyError("no library %r: LIBRARIES, LATER_LIBRARIES and OPEN_LIBRARIES have %s" % (name, ", ".join(r.name for r in all_libraries())))


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


def _headers():
    """csrc/*.hpp and the public headers: inputs of every object of every library."""
    return [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".hpp")] + [row.header for row in all_libraries()]


def source_digest():
    """Content hash of everything the libraries are built from: the sources of every row of all_libraries(), csrc/*.hpp,
    include/*.h, the compiler path and the flags."""
    return _digest([os.path.join(row.dir, s) for row in all_libraries() for s in row.sources] + _headers(), [_hipcc()] + FLAGS)


LAST_BUILD = {"mode": None, "digest": None, "compiled": [], "linked": []}      # what the last build() call did: "compiled" | "linked" | "reused"


def build(force=False, verbose=True):
    """Builds every library of all_libraries(); -> the path of libemrt_hip.so (the others are library(name).lib).  Only the objects whose inputs changed
    are compiled, and only the libraries that hold one of them are linked again."""
    hipcc = _hipcc()
    hdrs = _headers()
    objs, jobs = {row.lib: [] for row in all_libraries()}, []
    for _, lib, d, sources, _ in all_libraries():
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
    for lib in objs:
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
