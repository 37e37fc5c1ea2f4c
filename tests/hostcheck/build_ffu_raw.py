"""Builds tests/hostcheck/libhostcheck_ffu_raw.so: the unsaturated products of csrc/ffu.h on raw limbs, compiled for the HOST with the
bound assertions live (test-only; one translation unit, apart from libhostcheck.so)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "tokamak-zk-evm_amd", "csrc")
SRC = os.path.join(HERE, "hostcheck_ffu_raw.cpp")
SO = os.path.join(HERE, "libhostcheck_ffu_raw.so")


def stale():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("ff.h", "field_params.h", "ffu.h")]
    return not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps)


def build(force=False):
    """returns the path of the library, or None when hipcc is missing"""
    if not force and not stale():
        return SO
    if shutil.which("hipcc") is None:
        return None
    subprocess.run(["hipcc", "-O1", "-fPIC", "-shared", "--offload-host-only", "-I" + CSRC, SRC, "-o", SO], check=True)
    return SO
