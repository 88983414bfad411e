"""Build the in-tree HIP library vanrijn_amd/lib/libvanrijn_amd.so for gfx950 (hipcc).

    python -m vanrijn_amd.build [--force]                    # the product library
    python -m vanrijn_amd.build --out PATH [flags...]        # a variant library: the product flags, then these
    python -m vanrijn_amd.build --rev REV --out PATH [flags...]   # a git revision's csrc and include, this tree's flags
--print-flags, --print-sources, --print-render-sources: what a build would use, on one line; build nothing."""
import argparse
import concurrent.futures
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIB_DIR, "libvanrijn_amd.so")
# The units that include vr_render_kernel.h, one per camera mode: each takes minutes where every other unit
# takes seconds, so they come first (the lens mode's, which has the most code, at the head)
RENDER_SOURCES = ["vr_render_cam2.hip", "vr_render_cam1.hip", "vr_render_cam0.hip"]
SOURCES = RENDER_SOURCES + [
    "vr_reproject.hip", "vr_host_reproject.cpp", "vr_denoise.hip", "vr_host_denoise.cpp", "vr_features.hip", "vr_render_launch.hip", "vr_reduce.hip", "vr_cull.hip", "vr_query.hip", "vr_integrate.hip", "vr_image.hip",
    "vr_build.hip", "vr_refit.hip", "vr_host.cpp", "vr_host_bvh.cpp", "vr_host_scene.cpp", "vr_host_edit.cpp", "vr_host_rays.cpp",
    "vr_host_film.cpp", "vr_host_io.cpp"]
# compilers at a time: a unit compiles on one core, and a machine may report more cores than a job may use
JOBS = min(16, os.cpu_count() or 1)

FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-shared",
    # Rust never contracts a*b+c into an FMA; neither may we
    "-ffp-contract=off",
    "-fno-fast-math",
    "-Wall",
    # the AMDGPU register-pressure trackers in the machine scheduler: the same registers (168, no
    # scratch) and bit-identical records, C3's render kernel 37.49 -> 37.06 ms (-1.2 %), C5 -0.2 %
    # (profiles/r06/sched/)
    "-Xarch_device",
    "-mllvm=-amdgpu-use-amdgpu-trackers",
]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    inputs = [f for pat in ("*.hip", "*.cpp", "*.h") for f in glob.glob(os.path.join(CSRC, pat))]
    inputs += [os.path.join(HERE, "..", "include", "vanrijn_amd.h"), os.path.abspath(__file__)]  # (this file: the flags)
    return any(os.path.getmtime(f) > t for f in inputs)


def compile_flags_of():
    """The per-source compile flags of the product build (FLAGS without the link-only -shared): every
    variant library and every analysis tool takes them from here, so it differs from the product only in
    what the experiment changes."""
    return [f for f in FLAGS if f != "-shared"]


def compile_units(paths, out_dir, flags, suffix=".o", verbose=False, quiet=False):
    """hipcc `flags` on each of `paths` into out_dir/<name><suffix>, at most JOBS compilers at a time,
    started in the order given.  Returns the outputs in that order."""
    def one(path):
        out = os.path.join(out_dir, os.path.splitext(os.path.basename(path))[0] + suffix)
        cmd = [hipcc()] + flags + [path, "-o", out]
        if verbose:
            print(" ".join(cmd), flush=True)
        if subprocess.call(cmd, stderr=subprocess.DEVNULL if quiet else None) != 0:
            raise subprocess.CalledProcessError(1, cmd)
        return out
    with concurrent.futures.ThreadPoolExecutor(JOBS) as pool:
        return list(pool.map(one, paths))


def build_library(out, sources=SOURCES, flags=(), csrc=CSRC, verbose=False):
    """`sources` of the directory `csrc` compiled with the product flags and then `flags`, each to its own
    object (no device-side linking is needed: every kernel is launched from its own translation unit),
    then one shared-library link into `out`."""
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        objs = compile_units([os.path.join(csrc, s) for s in sources], tmp, compile_flags_of() + list(flags) + ["-c"],
                             verbose=verbose)
        link = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-lz", "-o", out + ".tmp"]
        if verbose:
            print(" ".join(link), flush=True)
        subprocess.check_call(link)
    os.replace(out + ".tmp", out)
    return out


def build_revision(rev, out, flags=(), verbose=False):
    """The library of a git revision's csrc and include, for A/B against the working tree: that revision's
    own translation units (it may have fewer, or one render unit), this tree's flags on both sides."""
    root = os.path.dirname(HERE)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.check_output(["git", "-C", root, "archive", rev, "vanrijn_amd/csrc", "include"])
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        csrc = os.path.join(tmp, "vanrijn_amd", "csrc")
        units = [f for f in os.listdir(csrc) if f.endswith((".hip", ".cpp"))]
        units.sort(key=lambda f: (not f.startswith("vr_render"), f))  # the long ones first
        return build_library(out, units, flags, csrc, verbose)


def build(force=False, verbose=False):
    if not force and not stale():
        return LIB
    # VR_TUNING=1: the occupancy-variant kernels of tools/variants.py
    return build_library(LIB, flags=["-DVR_TUNING_VARIANTS"] if os.environ.get("VR_TUNING") == "1" else [],
                         verbose=verbose)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(allow_abbrev=False)
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--rev")
    for what in ("flags", "sources", "render-sources"):
        ap.add_argument("--print-" + what, action="store_true")
    opt, extra = ap.parse_known_args()  # what is left: compile flags of a variant
    if opt.print_flags:
        print(" ".join(compile_flags_of()))
    elif opt.print_sources:
        print(" ".join(SOURCES))
    elif opt.print_render_sources:
        print(" ".join(RENDER_SOURCES))
    elif opt.rev:
        print(build_revision(opt.rev, opt.out or ap.error("--rev needs --out"), extra, verbose=True))
    elif opt.out:
        print(build_library(opt.out, flags=extra, verbose=True))
    else:
        print(build(force=opt.force, verbose=True))
