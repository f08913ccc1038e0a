# the short-randomness mix's host-mirror test (tests/test_gpu_smix_cpp.py builds it: make -C tests/cpp -f smix.mk), by the pattern of
# test_mix; it links the HIP library alone
ROOT := ../..
CXX ?= g++
test_smix: test_smix.cpp $(ROOT)/paillier_halo2_amd/host/paillier_chip.hpp $(ROOT)/paillier_halo2_amd/host/benes.hpp $(ROOT)/paillier_halo2_amd/host/biguint.hpp
	$(CXX) -O2 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ test_smix.cpp -L/opt/rocm/lib -lamdhip64 -L$(ROOT)/paillier_halo2_amd/csrc -lpz_hip \
	  -Wl,-rpath,'$$ORIGIN/../../paillier_halo2_amd/csrc' -Wl,-rpath,/opt/rocm/lib
