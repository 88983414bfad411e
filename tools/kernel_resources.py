"""VGPR / SGPR / scratch / LDS of the render-kernel instantiations (analysis aid), or of the
ray-query / integrate kernels' when given vr_query.hip / vr_integrate.hip.  A render kernel is named by its
template arguments by name (tools/isa_sections.py kernel_args), whichever revision the source is.
    python tools/kernel_resources.py [--asm FILE] [other/vr_render.hip | vanrijn_amd/csrc/vr_query.hip] [extra hipcc flags]
--asm: read this device assembly instead of compiling."""
import os
import re
import subprocess
import sys
import tempfile

from isa_sections import kernel_args, kernel_label

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    if sys.argv[1:2] == ["--asm"]:
        return report(sys.argv[2])
    out = os.path.join(tempfile.mkdtemp(), "render.s")
    # the product build's compile flags (vanrijn_amd/build.py FLAGS): the scheduler options change registers
    flags = subprocess.check_output([sys.executable, os.path.join(ROOT, "vanrijn_amd/build.py"), "--print-flags"],
                                    text=True).split()
    extra = sys.argv[1:]
    src = os.path.join(ROOT, "vanrijn_amd/csrc/vr_render.hip")
    if extra and extra[0].endswith(".hip"):  # another revision's source (e.g. from git archive)
        src, extra = extra[0], extra[1:]
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-S"] + extra + [src, "-o", out],
                          stderr=subprocess.DEVNULL)
    report(out)


def report(asm):
    meta = open(asm).read().split("amdhsa.kernels:")[1]
    for blk in re.split(r"\n  - ", meta):
        name = re.search(r"\.name:\s+(\S+)", blk)
        args = name and re.search(r"(?:render|query|integrate)_kernelIL(.*?)EEEv", name.group(1))
        if not args:
            continue
        render = kernel_args(name.group(1))
        args = kernel_label(render)[len("render_kernel"):] if render else (
            ("query " if "query_kernel" in name.group(1) else "integrate ") + args.group(1))
        f = {k: re.search(r"\." + k + r":\s+(\d+)", blk) for k in
             ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
              "group_segment_fixed_size")}
        print("%-112s vgpr %3s sgpr %3s sgpr_spill %3s scratch %4s lds %6s" % (
            args, f["vgpr_count"].group(1), f["sgpr_count"].group(1), f["sgpr_spill_count"].group(1),
            f["private_segment_fixed_size"].group(1), f["group_segment_fixed_size"].group(1)))


if __name__ == "__main__":
    main()
