# the t-of-T threshold decryption's host-mirror test (tests/test_gpu_shamir_cpp.py builds it: make -C tests/cpp -f shamir.mk), by the
# pattern of test_partial; it links the HIP library alone
ROOT := ../..
CXX ?= g++
test_shamir: test_shamir.cpp $(ROOT)/paillier_halo2_amd/host/paillier_chip.hpp $(ROOT)/paillier_halo2_amd/host/biguint.hpp
	$(CXX) -O2 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ test_shamir.cpp -L/opt/rocm/lib -lamdhip64 -L$(ROOT)/paillier_halo2_amd/csrc -lpz_hip \
	  -Wl,-rpath,'$$ORIGIN/../../paillier_halo2_amd/csrc' -Wl,-rpath,/opt/rocm/lib
