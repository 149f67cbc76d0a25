# Drop-in proof: the reference's OWN test sources (test/*.cpp, Catch2), compiled
# UNMODIFIED from where they lie under $(REF) against include/gtn (the header-only
# C++ mirror) and linked against libgtn_amd.so (HIP, gfx950).
# Outputs go to oracle/_ref/dropin/ (git-ignored, kept with the rest of _ref/ where the
# reference is absent); no reference source is copied into the repo.
# tests/test_dropin_gpu.py runs them.  Run by __graft_entry__.build() where $(REF) exists:
#   make -C oracle dropin
ifndef REF
$(error REF: the reference checkout -- run as `make -C oracle dropin`)
endif
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)..)
BIN := $(HERE)_ref/dropin
TESTS := graph_test functions_test autograd_test creations_test criterion_test parallel_test rand_test utils_test
CXX ?= g++
CXXFLAGS := -O1 -std=c++17 -DCATCH_CONFIG_NO_POSIX_SIGNALS -I$(ROOT)/include -I$(REF)/test
LDFLAGS := -L$(ROOT)/gtn_amd/lib -lgtn_amd -Wl,-rpath,'$$ORIGIN/../../../gtn_amd/lib' -pthread

# ... and the two examples and two benchmarks that ARE callers of the hot path (examples/ctc.cpp, examples/asg.cpp,
# benchmarks/ctc.cpp, benchmarks/functions.cpp: SURVEY.md section 8(b)), equally unmodified.  The reference's other
# examples and benchmarks are outside section 8 and are not built (`make EXAMPLES="asg ctc tutorial ..."` still
# builds any of them).  tests/test_dropin_cpu.py runs the examples on the CPU host.
# (The repository's own native test programs, tests/native/*.cpp, are built by tests/dropin/Makefile.)
EXAMPLES := asg ctc
BENCHES := ctc functions

all: $(addprefix $(BIN)/,$(TESTS)) $(addprefix $(BIN)/ex_,$(EXAMPLES)) $(addprefix $(BIN)/bm_,$(BENCHES))

$(BIN)/ex_%: $(REF)/examples/%.cpp $(wildcard $(ROOT)/include/gtn/*.h) $(ROOT)/include/gtn_amd.h
	@mkdir -p $(BIN)
	$(CXX) -O1 -std=c++17 -I$(ROOT)/include -I$(REF) $< $(LDFLAGS) -o $@

$(BIN)/bm_%: $(REF)/benchmarks/%.cpp $(wildcard $(ROOT)/include/gtn/*.h) $(ROOT)/include/gtn_amd.h
	@mkdir -p $(BIN)
	$(CXX) -O1 -std=c++17 -I$(ROOT)/include -I$(REF) $< $(LDFLAGS) -o $@

$(BIN)/%: $(REF)/test/%.cpp $(wildcard $(ROOT)/include/gtn/*.h) $(ROOT)/include/gtn_amd.h
	@mkdir -p $(BIN)
	$(CXX) $(CXXFLAGS) $< $(LDFLAGS) -o $@

clean:
	rm -rf $(BIN)
.PHONY: all clean
