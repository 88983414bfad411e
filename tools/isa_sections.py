"""Static VALU cost of the render kernel per code section (analysis aid).

Builds the camera unit of the instantiation asked for (vr_render_cam<CAM>.hip) to assembly with the product
build's flags and -DVR_MARKS (asm ';@mark <name>' comments at the section starts of vr_render_kernel.h),
takes that instantiation of render_kernel, selected by
its template arguments, attributes every instruction to the last marker above it in layout order, and
prices each instruction with a simple gfx950 issue model (wave64: f32 / int VALU 2 cycles, f64 and 64-bit
ops 4, f64 transcendentals 16, 32-bit integer multiplies 8).  The kernel's resources (VGPRs, SGPRs,
scratch, LDS, occupancy) are printed first.
    python tools/isa_sections.py [NAME=VALUE ...] [--asm FILE] [--keep FILE] [other/vr_render.hip] [extra hipcc flags]
NAME: a template parameter of render_kernel (PARAMS below); the defaults are the C3 timed kernel: STACK 32,
Lambertian-only, DARK0, 16-bit stack entries, the default camera, the single-BVH instantiation
(ONE=0: the generic kernel).  --asm: read this assembly (built with -DVR_MARKS) instead of compiling;
--keep: leave the assembly there.  An older source, whose kernel has fewer template parameters, is
matched on the parameters it has."""
import collections
import importlib.util
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# render_kernel's template parameters in order, with the kind of each as a name spells it (i: int, b: bool)
PARAMS = ["STACK", "COUNT", "RECORD", "DARK0", "MATS", "MINW", "WHITTED", "COOP", "BIG", "S16", "CAM", "ONE"]
KINDS = "ibbbiibbbbib"
# ... and of the sources up to round 13, whose kernel had the split probe's TRACE after BIG; a source older
# still has a prefix of this list (the parameters were added at the end)
PARAMS_R13 = PARAMS[:9] + ["TRACE"] + PARAMS[9:]
KINDS_R13 = KINDS[:9] + "b" + KINDS[9:]
# the language's defaults of the parameters added over time
DEFAULTS = {"MATS": 3, "MINW": 3, "WHITTED": 0, "COOP": 0, "BIG": 0, "S16": 0, "CAM": 0, "ONE": 0}
# the C3 timed kernel
C3 = {"STACK": 32, "COUNT": 0, "RECORD": 0, "DARK0": 1, "MATS": 1, "MINW": 3, "WHITTED": 0, "COOP": 0, "BIG": 0,
      "S16": 1, "CAM": 0, "ONE": 1}
# the units besides the render units that hold a kernel vr_render.hip once held
MOVED_SOURCES = ["vr_reduce.hip", "vr_cull.hip", "vr_query.hip"]


def product_build():
    """vanrijn_amd/build.py as a module: its flags, unit lists and capped parallel compile, without importing
    the package (which loads the library)"""
    spec = importlib.util.spec_from_file_location("vr_build", os.path.join(ROOT, "vanrijn_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_assembly(out, extra, sources=None):
    """The device assembly of `sources` (paths), or of every unit that holds a kernel of the render launch, the
    ray trace or the reduce, with the product build's flags (the scheduler options change the code) and then
    `extra`: compiled in parallel under the build's cap, concatenated into `out`."""
    vb = product_build()
    if sources is None:
        sources = [os.path.join(vb.CSRC, s) for s in vb.RENDER_SOURCES + MOVED_SOURCES]
    with tempfile.TemporaryDirectory() as tmp:
        parts = vb.compile_units(sources, tmp, vb.compile_flags_of() + ["--cuda-device-only", "-S"] + extra, ".s",
                                 quiet=True)
        with open(out, "w") as f:
            for part in parts:
                f.write(open(part).read())


def kernel_args(name):
    """The template arguments of a render_kernel instantiation by parameter name, or None for another symbol.
    `name`: the mangled symbol (an assembly file's) or the demangled one (a rocprofv3 trace's).  The kinds of
    the arguments tell which source the name is from: today's 12, or an older one's (PARAMS_R13 or a prefix
    of it), whose missing parameters take their defaults and whose TRACE is kept only where it is set, so
    that a kernel from before the parameter left pairs with the same kernel after."""
    m = re.match(r"_ZN2vr3dev13render_kernelI((?:L[ib]n?\d+E)+)E", name)
    if m:
        found = re.findall(r"L([ib])(\d+)E", m.group(1))
    else:
        m = re.search(r"render_kernel<([^<>]*)>", name)
        if not m:
            return None
        found = [("i", v) if v.isdigit() else ("b", str(int(v == "true"))) for v in re.split(r",\s*", m.group(1).strip())]
    kinds = "".join(k for k, _ in found)
    names = PARAMS if kinds == KINDS else PARAMS_R13[:len(found)]
    if names is not PARAMS and kinds != KINDS_R13[:len(found)]:
        raise ValueError("render_kernel arguments of no known source: " + name)
    args = dict(DEFAULTS)
    args.update((p, int(v)) for p, (_, v) in zip(names, found))
    if not args.get("TRACE"):
        args.pop("TRACE", None)
    return args


def kernel_label(args):
    """render_kernel<NAME value, ...> of kernel_args' result: one string per instantiation, for keys and printing"""
    return "render_kernel<%s>" % ", ".join("%s %d" % (p, args[p]) for p in PARAMS_R13 if p in args)


def kernel_bodies(text):
    """{mangled name: instruction lines (markers kept)} of the render_kernel instantiations of an assembly file."""
    out, name = {}, None
    for l in text.split("\n"):
        if name is None:
            m = re.match(r"(_ZN2vr3dev13render_kernelI\w+):", l)
            if m:
                name = m.group(1)
                out[name] = []
            continue
        if l.startswith(".Lfunc_end"):
            name = None
            continue
        t = l.strip()
        if ";@mark" in t:
            out[name].append(t)
            continue
        t = t.split(";")[0].strip()
        if not t or t.startswith(".") and not t.endswith(":"):
            continue
        out[name].append(t)
    return out


def resources(text, name):
    """The kernel's metadata: registers, scratch, LDS; and the occupancy the compiler notes below its code."""
    blk = next(b for b in re.split(r"\n  - ", text.split("amdhsa.kernels:")[1]) if re.search(r"\.name:\s+" + name + r"\s", b))
    f = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in
         ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")}
    tail = text[text.index("\n" + name + ":"):]
    occ = re.search(r";\s*Occupancy:\s*(\d+)", tail)
    f["occupancy"] = int(occ.group(1)) if occ else -1
    return f


def cost(op):
    if not op.startswith("v_"):
        return 0
    if re.match(r"v_(rcp|rsq|sqrt|exp|log|sin|cos|frexp_mant|frexp_exp)_f64", op):
        return 16
    if "f64" in op or "_u64" in op or "_i64" in op or "b64" in op and op.startswith("v_lshl") or op.startswith("v_pk_"):
        return 4
    if re.match(r"v_mul_(lo|hi)_(u|i)32|v_mad_(u|i)64", op):
        return 8
    return 2


def main():
    argv = sys.argv[1:]
    want, asm, keep, src = dict(C3), None, None, None
    extra = []
    while argv:
        a = argv.pop(0)
        if re.match(r"[A-Z0-9]+=\d+$", a) and a.split("=")[0] in PARAMS:
            want[a.split("=")[0]] = int(a.split("=")[1])
        elif a == "--asm":
            asm = argv.pop(0)
        elif a == "--keep":
            keep = argv.pop(0)
        elif a.endswith(".hip"):  # another revision's source (e.g. from git archive)
            src = a
        else:
            extra.append(a)
    if asm is None:
        asm = keep or os.path.join(tempfile.mkdtemp(), "render.s")
        if src is None:  # the one unit that holds the instantiation
            src = os.path.join(ROOT, "vanrijn_amd/csrc/vr_render_cam%d.hip" % want["CAM"])
        device_assembly(asm, ["-DVR_MARKS"] + extra, [src])
    text = open(asm).read()
    bodies = kernel_bodies(text)
    names = [n for n in bodies if kernel_args(n) == want]
    if not names:
        sys.exit("no %s in %s" % (kernel_label(want), asm))
    name = names[0]
    print(kernel_label(want))
    r = resources(text, name)
    print("vgprs %d  sgprs %d  sgpr spills %d  vgpr spills %d  scratch %d B  lds %d B  occupancy %d" % (
        r["vgpr_count"], r["sgpr_count"], r["sgpr_spill_count"], r["vgpr_spill_count"], r["private_segment_fixed_size"],
        r["group_segment_fixed_size"], r["occupancy"]))
    sec = "entry"
    stats = collections.defaultdict(lambda: collections.Counter())
    ops = collections.defaultdict(lambda: collections.Counter())
    for t in bodies[name]:
        m = re.search(r";@mark (\w+)", t)
        if m:
            sec = m.group(1)
            continue
        if t.endswith(":"):
            continue
        op = t.split()[0]
        st = stats[sec]
        st["insts"] += 1
        ops[sec][op] += 1
        if op.startswith("v_"):
            st["valu"] += 1
            st["cycles"] += cost(op)
            if "f64" in op:
                st["f64"] += 1
        elif op.startswith("s_"):
            st["salu"] += 1
        if op.startswith(("global_", "buffer_", "flat_")):
            st["vmem"] += 1
        if op.startswith("ds_"):
            st["lds"] += 1
    total = collections.Counter()
    for st in stats.values():
        total.update(st)
    stats["(whole kernel)"] = total
    print("%-14s %6s %6s %6s %6s %7s %5s %5s" % ("section", "insts", "valu", "f64", "salu", "vcycles", "vmem", "lds"))
    for k, st in stats.items():
        print("%-14s %6d %6d %6d %6d %7d %5d %5d" % (k, st["insts"], st["valu"], st["f64"], st["salu"], st["cycles"],
                                                    st["vmem"], st["lds"]))
    for k in os.environ.get("VR_ISA_OPS", "").split(","):  # opcode histograms of these sections
        if k in ops:
            print("\n" + k + ": " + ", ".join("%s %d" % kv for kv in ops[k].most_common() if kv[0].startswith("v_")))


if __name__ == "__main__":
    main()
