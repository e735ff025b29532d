"""Resource notes of the chain-kernel instantiations in a built object.

Usage: python tools/resource_notes.py [hygeia_amd/lib/obj/tg_kernels.hip.o] > listing.txt

Pulls the gfx950 code object out of the object's fat binary and prints, per
tg_forward_kernel / tg_backward_kernel / sg_chain_kernel instantiation (so
tg_kernels_fo.hip.o, tg_kernels_trc.hip.o, tg_kernels_res.hip.o, sg_kernels.hip.o, sg_kernels_mm.hip.o,
sg_kernels_fo.hip.o, sg_kernels_fomm.hip.o and sg_kernels_fohst.hip.o list too; sg_sample_kernels.hip.o
lists sg_sample_kernel), the figures of its
`llvm-readelf --notes` metadata: VGPRs, AGPRs, SGPRs, VGPR / SGPR spills,
private segment bytes and static LDS bytes (the chain kernels' LDS is dynamic).
Two listings of two builds compare with diff: a change that must not move an
existing instantiation leaves its line as it was. Needs no GPU.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
          "private_segment_fixed_size", "group_segment_fixed_size")


def listing(obj: str) -> list[str]:
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
    kernels, cur = [], None
    for line in notes.splitlines():
        m = re.match(r"\s+(- )?\.(\w+):\s+(.*)", line)
        if not m:
            continue
        if m.group(1) and m.group(2) == "agpr_count":  # first key of a kernel's map (its arguments' maps start otherwise)
            cur = {}
            kernels.append(cur)
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip("'")
    rows = []
    for k in kernels:
        name = k.get("name", "")
        if not any(kernel in name for kernel in ("tg_forward_kernel", "tg_backward_kernel", "sg_chain_kernel",
                                                 "sg_sample_kernel")):
            continue
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r"\(.*", "", dem).replace("void hyg::", "").replace(" ", "")
        # as hyg_tg_kernel_name / hyg_tg_kernel_name_multi spell it: the seventh
        # argument (a multi-model build) is written only where it is true
        # tg_forward_kernel's eighth (REC) is written only where it is false (a
        # forward-only build, tg_kernels_fo.hip.o), and then the seventh as well;
        # its ninth (TRC) only where it is true (a traced build, tg_kernels_trc.hip.o)
        # its tenth (RES) only where it is true (a resuming build, tg_kernels_res.hip.o)
        dem = re.sub(r"^(tg_forward_kernel<(?:[^,]+,){8}[^,]+),false>$", r"\1>", dem)
        dem = re.sub(r"^(tg_forward_kernel<(?:[^,]+,){7}[^,]+),false>$", r"\1>", dem)
        dem = re.sub(r"^(tg_forward_kernel<(?:[^,]+,){6}[^,]+),true>$", r"\1>", dem)
        dem = re.sub(r"^(tg_[^<]+<(?:[^,]+,){5}[^,]+),false>$", r"\1>", dem)
        # sg_chain_kernel<KT,NB,PE,PHS[,MM]>: likewise its fifth (the four before it
        # stay as they are, so a build from before the flag lists the same names)
        # its eighth (HST) is written only where it is true (a history build,
        # sg_kernels_fohst.hip.o); the seven before it stay as they are
        dem = re.sub(r"^(sg_chain_kernel<(?:[^,]+,){6}[^,]+),false>$", r"\1>", dem)
        dem = re.sub(r"^(sg_chain_kernel<(?:[^,]+,){3}[^,]+),false>$", r"\1>", dem)
        rows.append(" ".join([dem] + [k[f] for f in FIELDS]))
    return sorted(rows)


if __name__ == "__main__":
    obj = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "hygeia_amd", "lib", "obj", "tg_kernels.hip.o")
    print("kernel vgpr agpr sgpr vgpr_spill sgpr_spill private_bytes static_lds_bytes")
    print("\n".join(listing(obj)))
