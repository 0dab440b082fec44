#!/bin/bash
# Build the micro-benchmarks for gfx950 (hipcc cross-compiles without a GPU); run them with
#   ./tools/ubench/lds_atomic   etc.
cd "$(dirname "$0")"
# standalone: no product source included
for f in lds_atomic lds_dma_m0 fma_f64_loop mfma_f32_loop mfma_vmem_mix mfma4_loop mfma_mix permlane_swap mfma_f32_shapes mfma_valu_overlap issue_cost asm_behind_mfma reg_canary gather_width; do
  /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -o $f $f.hip 2>&1 | grep -E "error"
done
# the stamp harnesses include a product kernel source: compiled with the product's flags for that source
# (esr_nerf_amd/build.py), so that they time the kernel the library runs
for h in fwd16_stamps:mlp_bf16 tone_stamps:tone_wgrad split_stamps:mlp_split ldsread_srcc:mlp_bf16; do
  f=${h%%:*}
  flags=$(python3 ../../esr_nerf_amd/build.py --flags ${h#*:}.hip) || exit 1
  eval /opt/rocm/bin/hipcc $flags -o $f $f.hip 2>&1 | grep -E "error"
done
ls -la
