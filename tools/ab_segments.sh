#!/bin/bash
# A/B of the segment kernel's load-ahead depth (csrc/segment_kernels.hip, VGT_SEGMENT_LOAD_AHEAD).
#   tools/ab_segments.sh build   on the build machine: one library per depth under build/segments_ab/ (only
#                                segment_kernels.hip is compiled again; the other objects are the product build's)
#   tools/ab_segments.sh run     on the GPU: tools/bench_segments.py once per library, records under
#                                profiles/segments/ab/ (override: AB_OUT)
# Run from the repository root, after `make -C voxelized_geometry_tools_amd/csrc`.
set -e -o pipefail
DEPTHS="${DEPTHS:-1 2 4 8}"
CSRC=voxelized_geometry_tools_amd/csrc
AB=build/segments_ab
case "$1" in
build)
  mkdir -p $AB
  HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
  FLAGS=$(make -s -C $CSRC --eval='print-hipflags: ; @echo $(HIPFLAGS)' print-hipflags)
  OTHERS=$(ls $CSRC/*.o | grep -v -e segment_kernels.o -e '/testing_')
  for d in $DEPTHS; do
    $HIPCC $FLAGS -DVGT_SEGMENT_LOAD_AHEAD=$d -Rpass-analysis=kernel-resource-usage -c $CSRC/segment_kernels.hip \
      -o $AB/segment_kernels_$d.o 2> $AB/resources_$d.txt
    $HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -Wl,--version-script=$CSRC/exports.map \
      -o $AB/libvgt_hip_ahead$d.so $OTHERS $AB/segment_kernels_$d.o -ldl
    echo "depth $d:" $(grep -E "VGPRs:|ScratchSize" $AB/resources_$d.txt | sed 's/.*remark: *//; s/ \[-R.*//' | tr '\n' ' ')
  done
  ;;
run)
  OUT=${AB_OUT:-profiles/segments/ab}
  mkdir -p $OUT
  for d in $DEPTHS; do
    VGT_HIP_LIB=$PWD/$AB/libvgt_hip_ahead$d.so timeout -k 10 ${AB_TIMEOUT:-240} python tools/bench_segments.py \
      --label "load-ahead $d" --out $OUT/bench_segments_ahead$d.json ${AB_ARGS:-}
  done
  ;;
*)
  echo "usage: $0 build|run" >&2
  exit 2
  ;;
esac
