# the ballot's host-mirror test (tests/test_gpu_ballot_cpp.py builds it: make -C tests/cpp -f ballot.mk), by the pattern of test_wtally
ROOT := ../..
CXX ?= g++
test_ballot: test_ballot.cpp $(ROOT)/paillier_halo2_amd/host/paillier_chip.hpp $(ROOT)/paillier_halo2_amd/host/biguint.hpp
	$(CXX) -O2 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ test_ballot.cpp -L/opt/rocm/lib -lamdhip64 -L$(ROOT)/paillier_halo2_amd/csrc -lpz_hip -L$(ROOT)/oracle -lpz_oracle \
	  -Wl,-rpath,'$$ORIGIN/../../paillier_halo2_amd/csrc' -Wl,-rpath,'$$ORIGIN/../../oracle' -Wl,-rpath,/opt/rocm/lib -fopenmp
