#!/usr/bin/env bash
# VGPR and SGPR counts, scratch, occupancy and LDS of every kernel in the
# wc_k_*.hip translation units (gfx950).  Optional argument: a regex over the
# names.  (The DELIVER instantiations of k_rx_verdict are the ones whose
# template list ends in `unsigned int __vector`: their record-array pack.)
cd "$(dirname "$0")/.."
obj=$(mktemp --suffix=.o)
trap 'rm -f "$obj"' EXIT
for f in warpcore_amd/csrc/wc_k_*.hip; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -c --offload-device-only \
        -Rpass-analysis=kernel-resource-usage -Iinclude -Iwarpcore_amd/csrc \
        "$f" -o "$obj" 2>&1
done |
    sed 's/.*remark: //; s/ \[-Rpass.*//' |
    awk '/Function Name/{name=$3} /SGPRs:/ && !/Spill/{s=$NF} /^ *VGPRs:/{v=$2} /ScratchSize/{sc=$NF} /Occupancy/{occ=$NF} /LDS Size/{print name, "vgpr", v, "sgpr", s, "scratch", sc, "occ", occ, "lds", $NF}' |
    c++filt |
    sed 's/(anonymous namespace):://g; s/void wc::k_cksum_//; s/void wc:://; s/(.*) vgpr/ vgpr/' |
    grep -E "${1:-.}"
