# The reference's Shamirshare unit tests over include/hbmpc_shares.hpp and the plain C99 caller of the integer-point host calls
# (tests/test_gpu_shamir_cpp.py runs it).
# Kept apart from Makefile so that what `make -C tests/cpp` builds stays as it is:  make -C tests/cpp -f shamir_units.mk
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/mpc-protocols_amd
all: test_shamir_units
test_shamir_abi.o: test_shamir_abi.c $(ROOT)/include/hbmpc_hip.h
	$(CC) -O1 -std=c99 -Wall -Wextra -pedantic -Werror -I$(ROOT)/include -c $< -o $@
test_shamir_units: test_shamir_units.cpp test_shamir_abi.o $(ROOT)/include/hbmpc_shares.hpp $(ROOT)/include/hbmpc_hip.h
	$(CXX) -O1 -std=c++17 -Wall -I$(ROOT)/include $< test_shamir_abi.o -o $@ -L$(LIBDIR) -lhbmpc_hip -Wl,-rpath,'$$ORIGIN/../../mpc-protocols_amd'
