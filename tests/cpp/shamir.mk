# The integer-point Shamir encode on the CPU under ASan + UBSan (tests/test_shamir_routes.py builds and runs it): the route planner
# (mpc-protocols_amd/csrc/shamir_route.hpp), the interpolation table over arbitrary points (tables.hpp: point_coeff_rows) and the
# arithmetic of one output exactly as the kernel runs it (shamir_arith.hpp).
# Kept apart from Makefile so that what `make -C tests/cpp` builds stays as it is:  make -C tests/cpp -f shamir.mk
CXX ?= g++
ROOT := $(abspath ../..)
CSRC := $(ROOT)/mpc-protocols_amd/csrc
all: shamir_dump
shamir_dump: shamir_dump.cpp $(CSRC)/shamir_route.hpp $(CSRC)/shamir_arith.hpp $(CSRC)/tables.hpp $(CSRC)/host_fr.hpp $(CSRC)/field_dispatch.hpp
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@
