# hbmpc_dev_take_rows: the rule that picks a slice's route and tile (mpc-protocols_amd/csrc/take_plan.hpp) on the CPU under ASan + UBSan
# (tests/test_take_routes.py builds and runs it).
# Kept apart from Makefile so that what `make -C tests/cpp` builds stays as it is:  make -C tests/cpp -f take.mk
CXX ?= g++
ROOT := $(abspath ../..)
CSRC := $(ROOT)/mpc-protocols_amd/csrc
all: take_routes_dump
take_routes_dump: take_routes_dump.cpp $(CSRC)/take_plan.hpp
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@
