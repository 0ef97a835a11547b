# The C++ Mul wrapper's test (include/hbmpc_pipelines.hpp at n = 4, t = 1, N = 5; tests/test_gpu_mul.py runs it).
# Kept apart from Makefile so that what `make -C tests/cpp` builds stays as it is:  make -C tests/cpp -f mul.mk
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/mpc-protocols_amd
all: test_mul_pipeline
test_mul_pipeline: test_mul_pipeline.cpp $(ROOT)/include/hbmpc_pipelines.hpp $(ROOT)/include/hbmpc_shares.hpp $(ROOT)/include/hbmpc_hip.h
	$(CXX) -O1 -std=c++17 -Wall -I$(ROOT)/include $< -o $@ -L$(LIBDIR) -lhbmpc_hip -Wl,-rpath,'$$ORIGIN/../../mpc-protocols_amd'
