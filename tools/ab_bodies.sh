#!/bin/bash
# A/B of the sphere-model kernel's pose staging (csrc/body_kernels.hip, VGT_BODY_STAGE_POSES): 0 = every lane gathers
# the 12 doubles of its own link's pose (the product), 1 = a group's link poses are copied into LDS cooperatively.
#   tools/ab_bodies.sh build   on the build machine: one library per variant under build/bodies_ab/ (only
#                              body_kernels.hip is compiled again; the other objects are the product build's)
#   tools/ab_bodies.sh run     on the GPU: tools/bench_bodies.py once per library and round, the variants alternating,
#                              records under profiles/bodies/ab/ (override: AB_OUT)
# Run from the repository root, after `make -C voxelized_geometry_tools_amd/csrc`.
set -e -o pipefail
VARIANTS="${VARIANTS:-0 1}"
ROUNDS="${ROUNDS:-2}"
CSRC=voxelized_geometry_tools_amd/csrc
AB=build/bodies_ab
case "$1" in
build)
  mkdir -p $AB
  HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
  FLAGS=$(make -s -C $CSRC --eval='print-hipflags: ; @echo $(HIPFLAGS)' print-hipflags)
  OTHERS=$(ls $CSRC/*.o | grep -v -e body_kernels.o -e '/testing_')
  for v in $VARIANTS; do
    $HIPCC $FLAGS -DVGT_BODY_STAGE_POSES=$v -Rpass-analysis=kernel-resource-usage -c $CSRC/body_kernels.hip \
      -o $AB/body_kernels_$v.o 2> $AB/resources_$v.txt
    $HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -Wl,--version-script=$CSRC/exports.map \
      -o $AB/libvgt_hip_stage$v.so $OTHERS $AB/body_kernels_$v.o -ldl
    echo "stage poses $v:" $(grep -E "VGPRs:|ScratchSize|LDS Size" $AB/resources_$v.txt | sed 's/.*remark: *//; s/ \[-R.*//' | tr '\n' ' ')
  done
  ;;
run)
  OUT=${AB_OUT:-profiles/bodies/ab}
  mkdir -p $OUT
  for round in $(seq 1 $ROUNDS); do
    for v in $VARIANTS; do
      VGT_HIP_LIB=$PWD/$AB/libvgt_hip_stage$v.so timeout -k 10 ${AB_TIMEOUT:-240} python tools/bench_bodies.py \
        --label "stage poses $v, round $round" --out $OUT/bench_bodies_stage${v}_round$round.json ${AB_ARGS:-}
    done
  done
  ;;
*)
  echo "usage: $0 build|run" >&2
  exit 2
  ;;
esac
