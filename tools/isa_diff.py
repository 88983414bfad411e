"""Compare the gfx950 ISA of the render launch's kernels between two builds (refactoring check): render_kernel
(the camera units of vanrijn_amd/build.py --print-render-sources), accumulate_kernel (vr_reduce.hip), the block
cull and compact (vr_cull.hip) and trace_kernel (vr_query.hip).

    python tools/isa_diff.py save BEFORE.s     # device assembly of the current source, every unit's in one file
    python tools/isa_diff.py diff BEFORE.s     # rebuild and list kernels whose instructions differ
    python tools/isa_diff.py files A.s B.s     # compare two assembly files as they are
Extra hipcc flags may follow the file name, after another revision's single vr_render.hip if that is what
to build; the other flags are the product build's (vanrijn_amd/build.py).  The units compile in parallel.
Comments, directives and labels' names are ignored; kernel-argument offsets and register numbers are
compared as written.  Data labels (c_exp_tab, c_rgbspec) are not kernels.  render_kernel instantiations are
matched by their template arguments by name (tools/isa_sections.py kernel_args): a file from before a
parameter existed, or from when the kernel still had one that has left, pairs with the same kernels of the
other file, and the rest are listed as added or missing.  A kernel that two units of one file emit is an
error."""
import os
import re
import sys
import tempfile

from isa_sections import device_assembly, kernel_args, kernel_label

# the kernels compared: not vr_query.hip's query_kernel, which has its own history, nor a unit's data labels
KERNELS = "render|accumulate|block_cull|block_compact|trace"


def build(out, extra):
    src = None
    if extra and extra[0].endswith(".hip"):  # another revision's source (e.g. from git archive)
        src, extra = [extra[0]], extra[1:]
    device_assembly(out, extra, src)


def kernels(path):
    out, cur = {}, None
    for line in open(path).read().split("\n"):
        m = re.match(r"^([_A-Za-z0-9]+):", line)
        if m and re.match(r"_ZN2vr3dev\d+(%s)_kernel" % KERNELS, m.group(1)):
            args = kernel_args(m.group(1))
            cur = kernel_label(args) if args else m.group(1)
            if cur in out:
                sys.exit("%s: %s is emitted twice" % (path, cur))
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        out[cur].append(re.sub(r"\.LBB\d+_\d+", "L", t))
    return out


def main():
    mode, path, extra = sys.argv[1], sys.argv[2], sys.argv[3:]
    if mode == "save":
        build(path, extra)
        return
    if mode == "files":
        now, extra = extra[0], extra[1:]
    else:
        now = os.path.join(tempfile.mkdtemp(), "now.s")
        build(now, extra)
    a, b = kernels(path), kernels(now)
    same = 0
    for k in sorted(set(a) | set(b)):
        if a.get(k) == b.get(k):
            same += 1
        elif k not in a:
            print("ADDED %s: %d instructions" % (k, len(b[k])))
        elif k not in b:
            print("MISSING %s: %d instructions" % (k, len(a[k])))
        else:
            print("DIFF %s: %d -> %d instructions" % (k, len(a[k]), len(b[k])))
    print("%d kernels before, %d after, %d identical, %d added, %d missing" % (
        len(a), len(b), same, len(set(b) - set(a)), len(set(a) - set(b))))


if __name__ == "__main__":
    main()
