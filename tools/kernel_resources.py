#!/usr/bin/env python3
"""development: the compiler's resource lines (-Rpass-analysis=kernel-resource-usage, gfx950, no GPU needed) of every kernel of
one csrc/*.hip file as a table: VGPRs, SGPRs, scratch bytes per lane, waves per SIMD, LDS bytes.
usage: tools/kernel_resources.py [--filter SUBSTRING] [--csrc DIR] lin_static.hip      (DIR: another checkout's csrc, for a before / after pair)"""
import argparse
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"TotalSGPRs": "SGPR", "VGPRs": "VGPR", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "waves", "LDS Size [bytes/block]": "LDS"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source")
    ap.add_argument("--filter", default="")
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ddp_pinocchio_amd", "csrc"))
    a = ap.parse_args()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(a.csrc, "..", "..", "include"),
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(a.csrc, a.source), "-o", os.path.join(tmp, "dev.o")]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for line in text.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            if filt:
                name = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))
            cur = {"name": name}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z]+(?: \[[^\]]*\]| Size \[[^\]]*\])?): (\d+)", line)
        if m and cur is not None and m.group(1) in KEYS:
            cur[KEYS[m.group(1)]] = int(m.group(2))
    for r in rows:
        if a.filter in r["name"]:
            print(f"{r['name']:72s} VGPR {r['VGPR']:3d}  SGPR {r['SGPR']:3d}  scratch {r['scratch']:5d} B  waves/SIMD {r['waves']}  LDS {r['LDS']:6d} B")


if __name__ == "__main__":
    main()
