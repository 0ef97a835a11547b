# BatchRecon: the planner's rule for hbmpc_[gl_]dev_batchrecon_parties on the CPU under ASan + UBSan (tests/test_batchrecon_routes.py builds
# and runs it), and the C++ BatchRecon wrapper's test (include/hbmpc_pipelines.hpp at n = 4, t = 1, d = 1, three chunks;
# tests/test_gpu_batchrecon_pipeline.py runs it).
# Kept apart from Makefile so that what `make -C tests/cpp` builds stays as it is:  make -C tests/cpp -f batchrecon.mk
CXX ?= g++
ROOT := $(abspath ../..)
CSRC := $(ROOT)/mpc-protocols_amd/csrc
LIBDIR := $(ROOT)/mpc-protocols_amd
all: batchrecon_routes_dump test_batchrecon_pipeline
batchrecon_routes_dump: batchrecon_routes_dump.cpp $(CSRC)/protocol_route.hpp $(CSRC)/field_dispatch.hpp
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@
test_batchrecon_pipeline: test_batchrecon_pipeline.cpp $(ROOT)/include/hbmpc_pipelines.hpp $(ROOT)/include/hbmpc_shares.hpp $(ROOT)/include/hbmpc_hip.h
	$(CXX) -O1 -std=c++17 -Wall -I$(ROOT)/include $< -o $@ -L$(LIBDIR) -lhbmpc_hip -Wl,-rpath,'$$ORIGIN/../../mpc-protocols_amd'
