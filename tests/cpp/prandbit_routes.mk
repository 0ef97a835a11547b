# CPU-only: the PRandBit / PRandInt calls' planner under ASan + UBSan (tests/test_prandbit_routes.py builds and runs it).
# Kept apart from Makefile so that what `make -C tests/cpp` builds stays as it is:  make -C tests/cpp -f prandbit_routes.mk
CXX ?= g++
ROOT := $(abspath ../..)
CSRC := $(ROOT)/mpc-protocols_amd/csrc
all: prandbit_routes_dump
prandbit_routes_dump: prandbit_routes_dump.cpp $(CSRC)/prandbit_route.hpp $(CSRC)/field_dispatch.hpp
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@
