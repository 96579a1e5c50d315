# The coarse-hull form of the plain X pass against the brute-force line transform, with the filter on and off
# (tests/test_sweep_coarse_hull.py): the sweep kernels compiled for the CPU like `sweep_emulation` in the Makefile next to
# this file, with the kernel's own assertions under VGT_HOST_EMULATION and its record of the rows the chord test drops.
#   make -f sweep_coarse_hull.mk [SWEEP_FLAGS="-DVGT_SWEEP_RING=64"] [COARSE_OUT=name]
CXX ?= g++
ROOT = ../..
PKG = $(ROOT)/voxelized_geometry_tools_amd
COARSE_OUT ?= sweep_coarse_hull_default
SWEEP_FLAGS ?=
$(COARSE_OUT): sweep_coarse_hull.cc hip_shim/hip/hip_runtime.h $(PKG)/csrc/edt_sweep_kernels.hip $(PKG)/csrc/edt_device.hpp
	$(CXX) -O2 -std=c++17 -x c++ -Wall -Wextra -Wno-unused-parameter -Wno-unused-function -Wno-unknown-pragmas -Ihip_shim -I$(ROOT)/include $(SWEEP_FLAGS) -o $@ sweep_coarse_hull.cc
