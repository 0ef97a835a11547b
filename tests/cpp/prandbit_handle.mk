# The C99 caller of the PRandBit / PRandInt handles and the C++ wrappers' test (tests/test_gpu_prandbit_parties.py builds and runs them).
# Kept apart from Makefile so that what `make -C tests/cpp` builds stays as it is:  make -C tests/cpp -f prandbit_handle.mk
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/mpc-protocols_amd
all: test_prandbit_handle test_prandbit_pipe
test_prandbit_handle: test_prandbit_handle.c $(ROOT)/include/hbmpc_hip.h
	$(CC) -O1 -std=c99 -Wall -Wextra -pedantic -I$(ROOT)/include $< -o $@ -L$(LIBDIR) -lhbmpc_hip -Wl,-rpath,'$$ORIGIN/../../mpc-protocols_amd'
test_prandbit_pipe: test_prandbit_pipe.cpp $(ROOT)/include/hbmpc_pipelines.hpp $(ROOT)/include/hbmpc_hip.h
	$(CXX) -O1 -std=c++17 -Wall -I$(ROOT)/include $< -o $@ -L$(LIBDIR) -lhbmpc_hip -Wl,-rpath,'$$ORIGIN/../../mpc-protocols_amd'
