# The C99 caller of the PRandBit / PRandInt entry points and the C++ compositions' test (tests/test_gpu_prandbit_abi.py builds and runs them).
# Kept apart from Makefile so that what `make -C tests/cpp` builds stays as it is:  make -C tests/cpp -f prandbit.mk
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/mpc-protocols_amd
all: test_prandbit_abi test_prandbit_pipeline
test_prandbit_abi: test_prandbit_abi.c $(ROOT)/include/hbmpc_hip.h
	$(CC) -O1 -std=c99 -Wall -Wextra -pedantic -I$(ROOT)/include $< -o $@ -L$(LIBDIR) -lhbmpc_hip -Wl,-rpath,'$$ORIGIN/../../mpc-protocols_amd'
test_prandbit_pipeline: test_prandbit_pipeline.cpp $(ROOT)/include/hbmpc_pipelines.hpp $(ROOT)/include/hbmpc_hip.h
	$(CXX) -O1 -std=c++17 -Wall -I$(ROOT)/include $< -o $@ -L$(LIBDIR) -lhbmpc_hip -Wl,-rpath,'$$ORIGIN/../../mpc-protocols_amd'
