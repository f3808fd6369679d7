#!/bin/bash
# Resource usage (VGPRs, SGPRs, LDS, scratch, occupancy) of every kernel from the compiler's remarks, with
# the Makefile's flags.
# usage: tools/kres.sh [csrc/file.hip ...] [-- extra hipcc flags]
# No file: every .hip under cuda-raytracer_amd/csrc that has kernels.  One line per kernel:
#   name  VGPRs SGPRs LDS[bytes/block] scratch[bytes/lane] waves/SIMD
cd "$(dirname "$0")/../cuda-raytracer_amd" || exit 1
files=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do files+=("$1"); shift; done
[ "$1" = "--" ] && shift
[ ${#files[@]} -eq 0 ] && files=($(grep -l __global__ csrc/*.hip))
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
for f in "${files[@]}"; do
  slp=""
  case "$(basename "$f")" in rt_render.hip|rt_query.hip) slp="-fno-slp-vectorize";; esac   # as the Makefile
  /opt/rocm/bin/hipcc -std=c++17 -O3 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math \
    -fno-gpu-flush-denormals-to-zero -fhip-fp32-correctly-rounded-divide-sqrt $slp -I../include -Ihost -Icsrc \
    --cuda-device-only -Rpass-analysis=kernel-resource-usage "$@" -c "$f" -o "$tmp/dev.o" 2>&1
done | c++filt | python3 -c '
import re, sys
rows, cur = {}, None
keys = {"VGPRs": "v", "TotalSGPRs": "s", "LDS Size [bytes/block]": "lds", "ScratchSize [bytes/lane]": "scr",
        "Occupancy [waves/SIMD]": "occ"}
for line in sys.stdin:
    m = re.search(r"remark: Function Name: (.*)$", line)
    if m:
        name = re.sub(r"\(anonymous namespace\)::|rtamd::|^void ", "", m.group(1).strip())
        name = re.sub(r"\(.*", "", name)
        while name in rows: name += " (again)"      # a kernel compiled in two files shows twice
        cur = rows.setdefault(name, {})
        continue
    m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
    if cur is not None and m and m.group(1) in keys: cur[keys[m.group(1)]] = int(m.group(2))
for name in sorted(rows):
    r = rows[name]
    if "v" in r: print("%-60s %3d %3d %6d %4d %2d" % (name, r["v"], r["s"], r["lds"], r["scr"], r["occ"]))'
