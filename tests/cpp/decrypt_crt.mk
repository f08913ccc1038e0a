# CRT decryption's host-mirror test (tests/test_gpu_decrypt_crt_cpp.py builds it: make -C tests/cpp -f decrypt_crt.mk), by the pattern of test_decrypt
ROOT := ../..
CXX ?= g++
test_decrypt_crt: test_decrypt_crt.cpp $(ROOT)/paillier_halo2_amd/host/paillier_chip.hpp $(ROOT)/paillier_halo2_amd/host/biguint.hpp
	$(CXX) -O2 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ test_decrypt_crt.cpp -L/opt/rocm/lib -lamdhip64 -L$(ROOT)/paillier_halo2_amd/csrc -lpz_hip -L$(ROOT)/oracle -lpz_oracle \
	  -Wl,-rpath,'$$ORIGIN/../../paillier_halo2_amd/csrc' -Wl,-rpath,'$$ORIGIN/../../oracle' -Wl,-rpath,/opt/rocm/lib -fopenmp
