# the threshold decryption's host-mirror test (tests/test_gpu_partial_cpp.py builds it: make -C tests/cpp -f partial.mk), by the pattern of
# test_ballot; it links the HIP library alone
ROOT := ../..
CXX ?= g++
test_partial: test_partial.cpp $(ROOT)/paillier_halo2_amd/host/paillier_chip.hpp $(ROOT)/paillier_halo2_amd/host/biguint.hpp
	$(CXX) -O2 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ test_partial.cpp -L/opt/rocm/lib -lamdhip64 -L$(ROOT)/paillier_halo2_amd/csrc -lpz_hip \
	  -Wl,-rpath,'$$ORIGIN/../../paillier_halo2_amd/csrc' -Wl,-rpath,/opt/rocm/lib
