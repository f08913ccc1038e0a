# the packed ballot's host-mirror test (tests/test_gpu_pballot_cpp.py builds it: make -C tests/cpp -f pballot.mk), by the pattern of
# test_sballot; it links the HIP library alone
ROOT := ../..
CXX ?= g++
test_pballot: test_pballot.cpp $(ROOT)/paillier_halo2_amd/host/paillier_chip.hpp $(ROOT)/paillier_halo2_amd/host/biguint.hpp
	$(CXX) -O2 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ test_pballot.cpp -L/opt/rocm/lib -lamdhip64 -L$(ROOT)/paillier_halo2_amd/csrc -lpz_hip \
	  -Wl,-rpath,'$$ORIGIN/../../paillier_halo2_amd/csrc' -Wl,-rpath,/opt/rocm/lib
