#!/usr/bin/env python3
"""Per-kernel register / scratch / occupancy table of one HIP source (hipcc -Rpass-analysis=kernel-resource-usage), CPU only.

    python tools/kernel_resources.py pixelpick_amd/csrc/acq_select.hip [name-filter]

The acquisition kernels are one source per stage: acq.hip (full-size scorers, list select), acq_topk.hip (selection on a score map),
acq_lowres.hip (scorers on the classifier-resolution logits, prob_at), acq_mc.hip (MC-dropout families), acq_select.hip.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    src = sys.argv[1]
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "pixelpick_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", "/dev/null"]
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
    cur = None
    rows = []
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()}
            rows.append(cur)
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    for r in rows:
        if flt in r["name"]:
            print(f"{r.get('vgpr', '?'):>4} vgpr {r.get('agpr', 0):>4} agpr {r.get('scratch', '?'):>5} scratch  occ {r.get('occ', '?')}  lds {r.get('lds', '?'):>6}  "
                  f"{r['name'].split('(')[0][:110]}")


if __name__ == "__main__":
    main()
