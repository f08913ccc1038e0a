# the weighted tally's host-mirror test (tests/test_gpu_wtally_cpp.py builds it: make -C tests/cpp -f wtally.mk), by the pattern of test_tally
ROOT := ../..
CXX ?= g++
test_wtally: test_wtally.cpp $(ROOT)/paillier_halo2_amd/host/paillier_chip.hpp $(ROOT)/paillier_halo2_amd/host/biguint.hpp
	$(CXX) -O2 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ test_wtally.cpp -L/opt/rocm/lib -lamdhip64 -L$(ROOT)/paillier_halo2_amd/csrc -lpz_hip -L$(ROOT)/oracle -lpz_oracle \
	  -Wl,-rpath,'$$ORIGIN/../../paillier_halo2_amd/csrc' -Wl,-rpath,'$$ORIGIN/../../oracle' -Wl,-rpath,/opt/rocm/lib -fopenmp
