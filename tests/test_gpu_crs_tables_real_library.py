"""gpu tier: the table checks of the CRS audit (bin/crs-check --circuit) on the reference's REAL 14-subcircuit library, assembled the way
tests/real_library.py does.  One `trusted-setup --fixed-tau`, the audit of what it wrote, and one swap of two eta records.  This is the
only test of the ownership rule (flat_wire_owners, host/tkmk_witness.hpp) on real flattenMaps, where several (subcircuit, wire) pairs map
to one flattened wire: if the honest reference string fails here, the rule is wrong, not the string."""
import os
import subprocess

import numpy as np
import pytest

import real_library

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "tokamak-zk-evm_amd", "bin")


def _run(cmd):
    env = {k: v for k, v in os.environ.items() if k not in ("TKMK_SUBCIRCUIT_LIBRARY", "TKMK_FR_ROOT_GENERATOR", "TKMK_PROVER_CHECK_CRS", "TKMK_CRS_AUDIT_SEED")}
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("crs_tables_real_library")
    library = real_library.assemble(str(tmp / "library"))
    crs = tmp / "crs"
    crs.mkdir()
    r = _run([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", library, "--output", str(crs), "--format", "tkcrs"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return {"library": library, "crs": str(crs), "tmp": tmp}


def _check(world, crs):
    r = _run([os.path.join(BIN, "crs-check"), "--crs", crs, "--subcircuit-library", world["library"], "--circuit"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.strip().splitlines()[-1], r.stderr


def test_honest_crs_of_the_real_library_passes(world):
    last, err = _check(world, world["crs"])
    assert last == "true", err
    for t in ("gamma", "eta", "delta", "delta_small", "alpha_chain", "singles"):
        assert "table %s " % t in err and "FAILED" not in err, err


def test_one_eta_swap_in_the_real_library_is_refused(world):
    from tkmk import crs as crsmod
    sp = real_library.setup_params()
    s_max, m_i = sp["s_max"], sp["l_D"] - sp["l"]
    sec = dict(crsmod.read_payload(os.path.join(world["crs"], "combined_sigma.tkcrs")))
    eta = bytearray(bytes(np.asarray(sec["eta_inv_li_o_inter_alpha4_kj"], np.uint8)))
    i, j = 3 * s_max + 5, (m_i - 2) * s_max + 5                              # the same column of two different interface wires
    a, b = bytes(eta[96 * i:96 * i + 96]), bytes(eta[96 * j:96 * j + 96])
    assert a != b and any(a) and any(b)
    eta[96 * i:96 * i + 96], eta[96 * j:96 * j + 96] = b, a
    sec["eta_inv_li_o_inter_alpha4_kj"] = bytes(eta)
    out = world["tmp"] / "eta_swapped"
    out.mkdir()
    open(out / "combined_sigma.tkcrs", "wb").write(crsmod.build_payload(sec))
    last, err = _check(world, str(out))
    assert last == "false" and "table eta:" in err and "table eta " in err, err
    assert err.count("FAILED") == 1, err
