#!/bin/bash
# Compiles the headline instantiations of the step kernel (NVP = 32, static Cassie topology: the row-capped fast one, MAXR = 31,
# that every stepping launch starts, and the full one, MAXR = 63, that finishes handed-over envs) and prints their register /
# scratch / LDS use.  FEAT=1 for the height-field instantiations; NVP=40 TOPO=TopoCassieTray38 FEAT=2 MAXRS=63 for the tray
# kernel; KEEP=file keeps the ISA of the last one (tools/asm_segments.py, tools/asm_liveness.py read it).
# FEAT holds the collision bits; the two other bits (pk_stages.h; the kernel's trailing SERVE parameter) are set as the product's tables have them: the row-capped fast
# forms (MAXR 31 / 47, not a list-walking pass) are LEAN -- neither FEAT_READOUT (4) nor FEAT_PROF (8) -- and every other form carries
# both -- except that the 40-dof model's two-wave fast form keeps FEAT_READOUT (kernels_tray_2w.hip says why).  PROF=1 compiles the fast form's profiled instantiation (+ FEAT_PROF: FORM_FAST_PROF / FORM_FAST_2W_PROF), SUMS=1 its sibling for launches that accumulate the step sums (+ FEAT_SUMS, 16: kernels_*_sums.hip), FULL=1 / FULL=0
# force both bits on / off whatever the form.
# SMALL=reward (or obs, probe, ...): instead, the kernels of csrc/<SMALL>_kernels.h, which are no templates, with the product's flags.
set -e
cd "$(dirname "$0")/.."
if [ -n "$SMALL" ]; then
T=$(mktemp -d)
printf '#include <hip/hip_runtime.h>\n#include "wave.h"\n#include "%s_kernels.h"\n' "$SMALL" > $T/one.hip
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 --offload-device-only -Iinclude -Icassie-mujoco-sim_amd/csrc \
  -ffp-contract=on ${SCHED--mllvm -amdgpu-sched-strategy=iterative-ilp} ${LICM--mllvm -disable-machine-licm} $EXTRA -Rpass-analysis=kernel-resource-usage ${KEEP:+-save-temps=obj} -c $T/one.hip -o $T/one.o 2>&1 |
  grep -E "Function Name|VGPRs:|AGPRs|Spill|ScratchSize|Occupancy|LDS Size|SGPRs:" | sed 's/.*remark: *//; s/ \[-Rpass.*//; s/^ \+/    /'
[ -n "$KEEP" ] && cp $T/one-hip-amdgcn-amd-amdhsa-gfx950.s "$KEEP" || true
rm -rf $T
exit 0
fi
for MAXR in ${MAXRS:-31 63}; do
T=$(mktemp -d)
LEAN=0; { [ "$MAXR" = 31 ] || [ "$MAXR" = 47 ]; } && [ "${WALK:-false}" = false ] && LEAN=1
[ -n "$FULL" ] && LEAN=$((1 - FULL))
KEEP_READOUT=0; [ "${NVP:-32}" = 40 ] && [ "${NW:-1}" = 2 ] && [ -z "$FULL" ] && KEEP_READOUT=4
SERVE=$(( LEAN ? (${PROF:-0} ? 8 : 0) | KEEP_READOUT | (${SUMS:-0} ? 16 : 0) : 12 ))
cat > $T/one.hip <<EOS
#include <hip/hip_runtime.h>
#include "wave.h"
#include "physics_kernel.h"
#include "topo_static.h"
template __global__ void ck::cassie_step_kernel<${NVP:-32}, ck::${TOPO:-TopoCassie32}, ${FEAT:-0}, $MAXR, ${NW:-1}, ${WALK:-false}, ${WPS:-${NW:-1}}, ${INROWS:-0}, $SERVE>(ck::PhysIO);
EOS
echo "cassie_step_kernel<${NVP:-32}, ${TOPO:-TopoCassie32}, FEAT=${FEAT:-0}, MAXR=$MAXR, NW=${NW:-1}, WALK=${WALK:-false}, WPS=${WPS:-${NW:-1}}${INROWS:+, INROWS=$INROWS}, SERVE=$SERVE>:"
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 --offload-device-only -Iinclude -Icassie-mujoco-sim_amd/csrc \
  -ffp-contract=on ${SCHED--mllvm -amdgpu-sched-strategy=iterative-ilp} ${LICM--mllvm -disable-machine-licm} $EXTRA -Rpass-analysis=kernel-resource-usage ${KEEP:+-save-temps=obj} -c $T/one.hip -o $T/one.o 2>&1 |
  grep -E "VGPRs:|AGPRs|Spill|ScratchSize|Occupancy|LDS Size|SGPRs:" | sed 's/.*remark: *//; s/ \[-Rpass.*//' | tail -8 | sed 's/^/    /'
[ -n "$KEEP" ] && cp $T/one-hip-amdgcn-amd-amdhsa-gfx950.s "$KEEP" || true
rm -rf $T
done
