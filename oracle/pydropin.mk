# The reference's OWN pybind11 binding (bindings/python/gtn/_*.cpp, seven modules + __init__.py), compiled UNMODIFIED
# from where it lies under /root/reference against include/gtn (the header-only C++ mirror) and linked to
# libgtn_amd.so: `import gtn` then IS the reference's Python package over the MI355X engine (SURVEY.md section 8(b):
# "callers recompile against the new headers").  Outputs only into oracle/_ref/py_ext/gtn/ (git-ignored, kept with the
# rest of _ref/ where the reference is absent); the package's __init__.py goes there as bytecode -- no reference
# source is copied into the repository.  tests/test_pydropin_gpu.py runs the reference's 47 Python tests and
# examples/pytorch_loss.py through it.  Run by __graft_entry__.build():  make -C oracle pydropin
ifndef REF
$(error REF: the reference checkout -- run as `make -C oracle pydropin`)
endif
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT := $(abspath $(HERE)..)
OUT := $(HERE)_ref/py_ext/gtn
PY ?= python3
SUF := $(shell $(PY)-config --extension-suffix 2>/dev/null || $(PY) -c "import sysconfig; print(sysconfig.get_config_var('EXT_SUFFIX'))")
PYINC := $(shell $(PY) -m pybind11 --includes)
MODS := _graph _functions _utils _creations _autograd _parallel _rand
CXX ?= g++
CXXFLAGS := -O1 -std=c++17 -shared -fPIC $(PYINC) -I$(ROOT)/include
LDFLAGS := -L$(ROOT)/gtn_amd/lib -lgtn_amd -Wl,-rpath,'$$ORIGIN/../../../../gtn_amd/lib' -pthread

all: $(addprefix $(OUT)/,$(addsuffix $(SUF),$(MODS))) $(OUT)/__init__.pyc

$(OUT)/%$(SUF): $(REF)/bindings/python/gtn/%.cpp $(wildcard $(ROOT)/include/gtn/*.h) $(ROOT)/include/gtn_amd.h
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) $< $(LDFLAGS) -o $@

$(OUT)/__init__.pyc: $(REF)/bindings/python/gtn/__init__.py
	@mkdir -p $(OUT)
	$(PY) -c "import py_compile; py_compile.compile('$<', cfile='$@', dfile='reference:bindings/python/gtn/__init__.py', doraise=True)"

clean:
	rm -rf $(HERE)_ref/py_ext
.PHONY: all clean
