"""Compare the gfx950 ISA of vr_render.hip's kernels between two builds (refactoring check).

    python tools/isa_diff.py save BEFORE.s     # device assembly of the current source
    python tools/isa_diff.py diff BEFORE.s     # rebuild and list kernels whose instructions differ
    python tools/isa_diff.py files A.s B.s     # compare two assembly files as they are
Extra hipcc flags may follow the file name; the others are the product build's (vanrijn_amd/build.py).
Comments, directives and labels' names are ignored; kernel-argument offsets and register numbers are
compared as written.  render_kernel instantiations are matched by their template arguments by name
(tools/isa_sections.py kernel_args): a file from before a parameter existed, or from when the kernel still
had one that has left, pairs with the same kernels of the other file, and the rest are listed as added or
missing."""
import os
import re
import subprocess
import sys
import tempfile

from isa_sections import kernel_args, kernel_label

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(out, extra):
    # the product build's compile flags (vanrijn_amd/build.py FLAGS): the scheduler options change the code
    flags = subprocess.check_output([sys.executable, os.path.join(ROOT, "vanrijn_amd/build.py"), "--print-flags"],
                                    text=True).split()
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-S"] + extra +
                          [os.path.join(ROOT, "vanrijn_amd/csrc/vr_render.hip"), "-o", out], stderr=subprocess.DEVNULL)


def kernels(path):
    out, cur = {}, None
    for line in open(path).read().split("\n"):
        m = re.match(r"^([_A-Za-z0-9]+):", line)
        if m and m.group(1).startswith("_ZN2vr3dev"):
            args = kernel_args(m.group(1))
            cur = kernel_label(args) if args else m.group(1)
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
