"""not-gpu tier: the root of unity under a NAMED generator and the process switch (include/tkmk.h:
bls12_381_get_root_of_unity_with_generator, tkmk_ntt_root_generator, tkmk_ntt_set_root_generator) — what lets a prover adopt the
convention a CRS was made under (tests/test_gpu_crs_root_identify.py) instead of trusting the declared constant.  Host arithmetic only.

Every "default" child has TKMK_FR_ROOT_GENERATOR REMOVED from its environment.  The oracle and pyref of a process are not switched by
tkmk_ntt_set_root_generator (they read the declared constant or the environment once), so the comparison against the oracle runs the
oracle in a child of its own under the oracle's override, never in the process that switched."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SIZES = (2, 4096, 1 << 23, 1 << 32)


def _root_int(g, n):
    """omega_n under generator g: g^((r-1)/2^32) squared down to order 2^ceil(log2 n)"""
    w = pow(g, (R - 1) >> 32, R)
    for _ in range(32 - (n - 1).bit_length()):
        w = w * w % R
    return w


def _child(code, gen=None):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tokamak-zk-evm_amd"), HERE, os.path.join(ROOT, "tools")]))
    env.pop("TKMK_FR_ROOT_GENERATOR", None)
    if gen is not None:
        env["TKMK_FR_ROOT_GENERATOR"] = str(gen)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("g", [5, 7])
@pytest.mark.parametrize("n", SIZES)
def test_named_generator_against_integers(tkmk, g, n):
    got = int.from_bytes(bytes(tkmk.get_root_of_unity_with_generator(g, n)), "little")
    assert got == _root_int(g, n)
    assert pow(got, n, R) == 1 and (n == 1 or pow(got, n // 2, R) == R - 1)


def test_named_generator_refuses_a_residue_and_degenerate_values(tkmk):
    for g in (4, 9, 1, 0):
        with pytest.raises(tkmk.TkmkError) as e:
            tkmk.get_root_of_unity_with_generator(g, 1 << 20)
        assert e.value.code == 11, g
    with pytest.raises(tkmk.TkmkError) as e:
        tkmk.get_root_of_unity_with_generator(5, (1 << 32) + 1)           # past the two-adicity, as get_root_of_unity
    assert e.value.code == 11


SWITCH_CODE = """
import json, tkmk
f = lambda b: int.from_bytes(bytes(b), "little")
out = {"before": tkmk.root_generator(), "root_before": f(tkmk.get_root_of_unity(4096))}
tkmk.set_root_generator(7)
out["after"] = tkmk.root_generator()
out["roots_after"] = {str(n): f(tkmk.get_root_of_unity(n)) for n in (2, 4096, 1 << 23, 1 << 32)}
try:
    tkmk.set_root_generator(4)
    out["residue"] = "accepted"
except tkmk.TkmkError as e:
    out["residue"] = e.code
out["after_refusal"] = tkmk.root_generator()
tkmk.set_root_generator(7)                                                # naming the generator in effect is a no-op
tkmk.set_root_generator(5)
out["back"] = [tkmk.root_generator(), f(tkmk.get_root_of_unity(4096))]
print(json.dumps(out))
"""


def test_switch_in_a_default_process():
    out = _child(SWITCH_CODE)
    assert out["before"] == 5 and out["root_before"] == _root_int(5, 4096)
    assert out["after"] == 7
    assert out["roots_after"] == {str(n): _root_int(7, n) for n in SIZES}
    assert out["residue"] == 11 and out["after_refusal"] == 7            # a refused set changes nothing
    assert out["back"] == [5, _root_int(5, 4096)]


def test_environment_gives_the_initial_value_only():
    out = _child(SWITCH_CODE, gen=7)
    assert out["before"] == 7 and out["root_before"] == _root_int(7, 4096) and out["after"] == 7
    assert out["back"] == [5, _root_int(5, 4096)]                         # a set wins over the environment


ORACLE_CODE = """
import json, oracle
print(json.dumps({str(n): oracle.to_ints(oracle.root_of_unity(n), 32)[0] for n in (2, 4096, 1 << 23, 1 << 32)}))
"""


def test_switched_product_equals_the_oracle_under_its_own_override():
    # the oracle in a child under ITS override; the product in a default child that switched: the two processes agree
    want = _child(ORACLE_CODE, gen=7)
    got = _child(SWITCH_CODE)["roots_after"]
    assert got == want
    assert _child(ORACLE_CODE) == {str(n): _root_int(5, n) for n in SIZES}   # and the default oracle is the declared generator's
