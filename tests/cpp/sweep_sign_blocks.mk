# Sweep 2's sign words on lines that straddle words and blocks (tests/test_sweep_sign_blocks.py): the sweep kernels compiled
# for the CPU like `sweep_emulation` in the Makefile next to this file, with the kernel's own assertions under
# VGT_HOST_EMULATION -- no use of a sign word that sweep 1 has not written for the item -- and the uses counted.
#   make -f sweep_sign_blocks.mk [SWEEP_FLAGS="-DVGT_SWEEP_BAND=8 -DVGT_SWEEP_RING=16 -DVGT_SWEEP_CHUNK=4"] [BLOCKS_OUT=name]
CXX ?= g++
ROOT = ../..
PKG = $(ROOT)/voxelized_geometry_tools_amd
BLOCKS_OUT ?= sweep_sign_blocks_default
SWEEP_FLAGS ?=
$(BLOCKS_OUT): sweep_sign_blocks.cc hip_shim/hip/hip_runtime.h $(PKG)/csrc/edt_sweep_kernels.hip $(PKG)/csrc/edt_device.hpp
	$(CXX) -O2 -std=c++17 -x c++ -Wall -Wextra -Wno-unused-parameter -Wno-unused-function -Wno-unknown-pragmas -Ihip_shim -I$(ROOT)/include $(SWEEP_FLAGS) -o $@ sweep_sign_blocks.cc
