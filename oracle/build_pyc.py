"""Compiles the reference's Python binding tests and its two Python examples (the PyTorch loss, the linear-chain CRF)
to bytecode where they lie (REF below: bindings/python/{test,examples}) into oracle/_ref/pyc/ -- git-ignored and
kept with the rest of oracle/_ref where the reference is absent: the reference's sources never enter the repository,
its compiled tests do.  tests/test_pydropin_gpu.py and tests/test_pydropin_cpu.py run them.  Run by
__graft_entry__.build() where the reference exists."""
import glob
import os
import py_compile
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/bindings/python"


def main():
    out = os.path.join(HERE, "_ref", "pyc")
    os.makedirs(out, exist_ok=True)
    srcs = sorted(glob.glob(os.path.join(REF, "test", "test_*.py"))) + \
        [os.path.join(REF, "examples", s) for s in ("pytorch_loss.py", "linear_crf.py")]
    for s in srcs:
        name = os.path.splitext(os.path.basename(s))[0]
        py_compile.compile(s, cfile=os.path.join(out, name + ".pyc"), dfile="reference:bindings/python/" + os.path.basename(s),
                           doraise=True)
    print("oracle/_ref/pyc:", len(srcs), "modules")


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit(0)
    main()
