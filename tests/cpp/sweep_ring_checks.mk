# Sweep 1's ring checks on lines that spill at every check (tests/test_sweep_ring_checks.py): the sweep kernels compiled for
# the CPU like `sweep_emulation` in the Makefile next to this file, with the kernel's own assertions under
# VGT_HOST_EMULATION -- a check spills one chunk or none -- and the spills counted.
#   make -f sweep_ring_checks.mk [SWEEP_FLAGS="-DVGT_SWEEP_BAND=8 -DVGT_SWEEP_RING=16 -DVGT_SWEEP_CHUNK=4"] [RING_OUT=name]
CXX ?= g++
ROOT = ../..
PKG = $(ROOT)/voxelized_geometry_tools_amd
RING_OUT ?= sweep_ring_checks_default
SWEEP_FLAGS ?=
$(RING_OUT): sweep_ring_checks.cc hip_shim/hip/hip_runtime.h $(PKG)/csrc/edt_sweep_kernels.hip $(PKG)/csrc/edt_device.hpp
	$(CXX) -O2 -std=c++17 -x c++ -Wall -Wextra -Wno-unused-parameter -Wno-unused-function -Wno-unknown-pragmas -Ihip_shim -I$(ROOT)/include $(SWEEP_FLAGS) -o $@ sweep_ring_checks.cc
