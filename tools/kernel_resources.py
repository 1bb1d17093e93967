#!/usr/bin/env python3
"""Resource usage of every kernel of one .hip file of the library, one line per kernel:
SGPRs, VGPRs, AGPRs, scratch, occupancy and LDS as the compiler reports them
(-Rpass-analysis=kernel-resource-usage), cross-compiled for gfx950 with the Makefile's flags
(no GPU needed).  Two listings of the same file, before and after a change, show whether
the kernels a change must not touch kept their registers and LDS:

    python tools/kernel_resources.py csrc/rt_dqn.hip > after.txt

The kernel names are demangled and sorted, so source line numbers do not enter the diff.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "reinforcement-light-rays-pathtracer_amd")
ROCM = os.environ.get("ROCM", "/opt/rocm")
# the Makefile's HIPFLAGS (+ DQNFLAGS for the rt_dqn*.hip files)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
         "-fno-slp-vectorize", "-fno-vectorize", "--offload-arch=gfx950", "-fno-gpu-rdc"]
DQN_FLAGS = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sgpr_spill"), ("VGPRs Spill", "vgpr_spill"),
          ("LDS Size [bytes/block]", "lds"))


def listing(src):
    flags = FLAGS + (DQN_FLAGS if os.path.basename(src).startswith("rt_dqn") else [])
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.path.join(ROCM, "bin", "hipcc"), *flags, "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "o.o")],
                           cwd=PKG, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    names = list(kernels)
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    dem = names
    if filt:
        dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    rows = []
    for mangled, name in zip(names, dem):
        name = re.sub(r"\(.*\)$", "", name.replace("rt::(anonymous namespace)::", ""))
        name = re.sub(r"^void ", "", name)
        rows.append(name + ": " + " ".join(f"{key}={kernels[mangled].get(key, '?')}" for _, key in FIELDS))
    return sorted(rows)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    print("\n".join(listing(sys.argv[1])))
