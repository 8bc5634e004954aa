#!/bin/bash
# round 4 visit 9: the vendor library on the box that measured the placements of the LDS-DMA pieces (the placement sweep went with the rejected placements)
R=$GRAFT_REPO_ROOT; cd $R; mkdir -p gpurun_out
timeout 300 python tools/vendor_gemm_compare.py 2>&1 | grep -v amdgpu.ids | tee gpurun_out/r04_v09_vendor.txt
