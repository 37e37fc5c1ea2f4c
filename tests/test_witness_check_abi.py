"""not-gpu tier: the witness check's symbols resolve, header and Python binding agree on the argument lists, and without a device the
entries fail loudly (TKMK_ERR_NO_DEVICE) instead of answering."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tokamak-zk-evm_amd", "bin")
KERNEL_ENTRIES = ("tkmk_witness_check_r1cs", "tkmk_witness_check_copy")
PROVER_ENTRIES = ("tkmk_witness_check_files", "tkmk_prover_check_witness")


def _prototype(header, name):
    """-> the C types of `name`'s parameters as the header declares them, names and comments dropped"""
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\btkmk_error\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, name + " is not declared in " + header
    out = []
    for param in m.group(1).split(","):
        param = " ".join(param.split())
        out.append(re.sub(r"\s*\b[a-z_0-9]+$", "", param).replace(" *", "*"))
    return out


def _ctype(c):
    if c.endswith("**") or c in ("tkmk_stream", "tkmk_prover*"):
        return ctypes.c_void_p if c != "char**" else ctypes.POINTER(ctypes.c_void_p)
    return {"const char*": ctypes.c_char_p, "int*": ctypes.POINTER(ctypes.c_int), "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
            "uint64_t*": ctypes.POINTER(ctypes.c_uint64), "const tkmk_fr*": ctypes.c_void_p, "const uint32_t*": ctypes.c_void_p,
            "uint32_t*": ctypes.c_void_p}[c]


def test_symbols_resolve(tkmk):
    from tkmk import service
    for name in KERNEL_ENTRIES:
        assert name in tkmk.SYMBOLS and hasattr(tkmk.lib(), name), name
    for testing in (False, True):
        for name in PROVER_ENTRIES:
            assert name in service.SYMBOLS and hasattr(service.lib(testing), name), name
    # the third prover-library surface of the check is the knob inside tkmk_prover_prove[_ex]: the same symbols as before
    assert hasattr(service.lib(), "tkmk_prover_prove_ex")


def test_header_and_binding_agree_on_the_argument_lists(tkmk):
    from tkmk import verify
    for name in KERNEL_ENTRIES:
        declared = _prototype("tkmk.h", name)
        assert [_ctype(c) for c in declared] == tkmk.WITNESS_CHECK_ARGTYPES[name], (name, declared)
    l = verify._lib()
    for name in PROVER_ENTRIES:
        declared = _prototype("tkmk_prover.h", name)
        assert [_ctype(c) for c in declared] == list(getattr(l, name).argtypes), (name, declared)
    assert _prototype("tkmk.h", "tkmk_witness_check_r1cs")[3:6] == ["uint32_t"] * 3            # n_rows, n_cols, stride
    assert _prototype("tkmk.h", "tkmk_witness_check_copy")[7:10] == ["uint64_t", "uint64_t*", "uint64_t*"]   # n_entries, the two host results


def test_binary_usage(tkmk):
    exe = os.path.join(BIN, "witness-check")
    for argv in ([], ["--synthesizer-stat"], ["--crs", "x", "--synthesizer-stat", "y"], ["--synthesizer-stat", "a", "--synthesizer-stat", "b"]):
        r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "Usage: witness-check --synthesizer-stat" in r.stderr and r.stdout == "", (argv, r)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("Usage: witness-check")


def test_no_device_is_an_error_not_a_verdict(tkmk, tmp_path):
    if tkmk.device_count() > 0:
        pytest.skip("a GPU is visible")
    import random

    import synth_circuit
    from tkmk import service, verify
    inst = synth_circuit.build(str(tmp_path), random.Random(83), s_max=8, n_gate_kinds=2, used_placements=8)
    ok, doc = ctypes.c_int(-1), ctypes.c_void_p()
    code = verify._lib().tkmk_witness_check_files(os.fsencode(inst["qap"]), os.fsencode(inst["synth"]), ctypes.byref(ok), ctypes.byref(doc))
    assert code == 12 and ok.value == 0 and not doc.value                  # TKMK_ERR_NO_DEVICE
    with pytest.raises(service.ProverError) as e:
        verify.witness_check(inst["qap"], inst["synth"])
    assert e.value.code == 12
    r = subprocess.run([os.path.join(BIN, "witness-check"), "--synthesizer-stat", inst["synth"], "--subcircuit-library", inst["qap"]], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "no HIP device" in r.stderr
    assert r.stdout.strip().splitlines()[-1] not in ("true", "false")
