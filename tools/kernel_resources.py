"""VGPR / SGPR / scratch / LDS of the render-kernel instantiations (analysis aid), or of the
ray-query / integrate / feature / denoise / reprojection kernels' when given vr_query.hip / vr_integrate.hip /
vr_features.hip / vr_denoise.hip / vr_reproject.hip.  A render kernel is named by its
template arguments by name (tools/isa_sections.py kernel_args), whichever revision the source is.
    python tools/kernel_resources.py [--asm FILE] [other/vr_render.hip | vanrijn_amd/csrc/vr_query.hip] [extra hipcc flags]
With no source: every unit that holds a kernel of the render launch (tools/isa_sections.py device_assembly),
compiled in parallel and read as one.  --asm: read this device assembly instead of compiling."""
import os
import re
import sys
import tempfile

from isa_sections import device_assembly, kernel_args, kernel_label


def main():
    if sys.argv[1:2] == ["--asm"]:
        return report(sys.argv[2])
    out = os.path.join(tempfile.mkdtemp(), "render.s")
    extra, src = sys.argv[1:], None
    if extra and extra[0].endswith(".hip"):  # one unit, or another revision's source (e.g. from git archive)
        src, extra = [extra[0]], extra[1:]
    device_assembly(out, extra, src)
    report(out)


def report(asm):
    for meta in open(asm).read().split("amdhsa.kernels:")[1:]:  # one list per unit
        for blk in re.split(r"\n  - ", meta.split(".end_amdgpu_metadata")[0]):
            report_kernel(blk)


def report_kernel(blk):
    name = re.search(r"\.name:\s+(\S+)", blk)
    args = name and re.search(r"(?:render|query|integrate|features)_kernelIL(.*?)EEEv", name.group(1))
    plain = name and re.search(r"\d+(denoise_\w+?_kernel|reproject_kernel)E", name.group(1))  # not a template: its own name
    if not args and not plain:
        return
    render = kernel_args(name.group(1)) if args else None
    args = plain.group(1) if plain else kernel_label(render)[len("render_kernel"):] if render else (
        re.search(r"(query|integrate|features)_kernel", name.group(1)).group(1) + " " + args.group(1))
    f = {k: re.search(r"\." + k + r":\s+(\d+)", blk) for k in
         ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")}
    print("%-112s vgpr %3s sgpr %3s sgpr_spill %3s scratch %4s lds %6s" % (
        args, f["vgpr_count"].group(1), f["sgpr_count"].group(1), f["sgpr_spill_count"].group(1),
        f["private_segment_fixed_size"].group(1), f["group_segment_fixed_size"].group(1)))


if __name__ == "__main__":
    main()
