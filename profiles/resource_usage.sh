#!/bin/bash
# Register / scratch / occupancy report of every k_wave_episodes and k_tuple_episodes instantiation, from the
# compiler (hipcc -Rpass-analysis=kernel-resource-usage, the product flags of th_rl_amd/build.py, device pass only):
#     profiles/resource_usage.sh [CSRC_DIR] > report.txt
# One line per kernel: mangled name, VGPRs, AGPRs, SGPRs, scratch bytes per lane, waves per SIMD, static LDS.
src=${1:-$(dirname "$0")/../th_rl_amd/csrc}
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
cd "$src" || exit 1
for f in thrl_wave_f32.hip thrl_wave_f32a.hip thrl_wave_f32c.hip thrl_wave_f32g.hip thrl_wave_f32n.hip thrl_wave_f32nc.hip thrl_wave_f32s.hip \
         thrl_wave_f64.hip thrl_wave_f64c.hip thrl_wave_f64g.hip thrl_wave_f64n.hip thrl_wave_f64nc.hip thrl_wave_f64s.hip \
         thrl_tuple_f32.hip thrl_tuple_f64.hip thrl_tuple_f32_noise.hip thrl_tuple_f64_noise.hip thrl_tuple_f32_sweep.hip \
         thrl_tuple_f64_sweep.hip; do
  ${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -Wno-pass-failed \
      --cuda-device-only -Rpass-analysis=kernel-resource-usage -c "$f" -o "$tmp/$f.o" 2> "$tmp/$f.log" &
done
wait
cat "$tmp"/*.log | python3 -c '
import re, sys
rows, cur = [], None
for line in sys.stdin:
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = {"f": m.group(1)}; rows.append(cur); continue
    for k in ("VGPRs", "AGPRs", "SGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]"):
        m = re.search(k + r": (\d+)", line)
        if m and cur is not None:
            cur[k.split()[0]] = m.group(1)
for r in sorted(rows, key=lambda r: r["f"]):
    if "episodes" in r["f"]:
        print("%s VGPR=%s AGPR=%s SGPR=%s scratch=%s occ=%s lds=%s" % (r["f"], r.get("VGPRs"), r.get("AGPRs"), r.get("SGPRs"),
              r.get("ScratchSize"), r.get("Occupancy"), r.get("LDS")))
'
