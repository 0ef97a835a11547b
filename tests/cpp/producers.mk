# RanSha / RanDouSha for all parties: the planner's rule for hbmpc_[gl_]dev_ransha_parties and hbmpc_[gl_]dev_randousha_parties on the CPU
# under ASan + UBSan (tests/test_producers_routes.py builds and runs it), and the test of the C++ wrappers hbmpc::ransha_parties /
# randousha_parties (include/hbmpc_pipelines.hpp at n = 4, t = 1, three columns; tests/test_gpu_producers_pipeline.py runs it).
# Kept apart from Makefile so that what `make -C tests/cpp` builds stays as it is:  make -C tests/cpp -f producers.mk
CXX ?= g++
ROOT := $(abspath ../..)
CSRC := $(ROOT)/mpc-protocols_amd/csrc
LIBDIR := $(ROOT)/mpc-protocols_amd
all: producers_routes_dump test_producers_pipeline
producers_routes_dump: producers_routes_dump.cpp $(CSRC)/protocol_route.hpp $(CSRC)/field_dispatch.hpp
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all $< -o $@
test_producers_pipeline: test_producers_pipeline.cpp $(ROOT)/include/hbmpc_pipelines.hpp $(ROOT)/include/hbmpc_shares.hpp $(ROOT)/include/hbmpc_hip.h
	$(CXX) -O1 -std=c++17 -Wall -I$(ROOT)/include $< -o $@ -L$(LIBDIR) -lhbmpc_hip -Wl,-rpath,'$$ORIGIN/../../mpc-protocols_amd'
