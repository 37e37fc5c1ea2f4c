"""gpu tier: the table checks of the CRS audit against the circuit (host/tkmk_crs_audit.hpp audit_tables: tkmk_crs_audit_circuit_files,
bin/crs-check --circuit, TKMK_PROVER_CHECK_CRS=2 at tkmk_prover_open).  The world of tests/test_gpu_crs_audit.py: one small circuit, one
`trusted-setup --fixed-tau`, tampered copies of the flat payload made with tkmk.crs.read_payload / build_payload.  Every tamper here keeps
every point valid and leaves xy_powers alone, so membership, the anchors and both ratio checks are clean and tkmk_crs_audit_files still
answers true: only the table checks can see them.  They run under three seeds through the testing library, the honest CRS beside them
under the same seed.  The prover's opens run in child processes."""
import json
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import g1_torsion as gt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "tokamak-zk-evm_amd", "bin")
SEEDS = (1, 0x9E3779B97F4A7C15, 2**64 - 59)
TABLES = ["gamma", "eta", "delta", "delta_small", "alpha_chain", "singles"]
OLD_KEYS = ["ok", "reason", "sections", "g2", "anchors", "ratio_y", "ratio_x"]


def _env(**extra):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tokamak-zk-evm_amd"), HERE, os.path.join(ROOT, "tools")]))
    for k in ("TKMK_FR_ROOT_GENERATOR", "TKMK_HOST_TRACE", "TKMK_PROVER_CHECK_CRS", "TKMK_CRS_AUDIT_SEED"):
        env.pop(k, None)
    env.update({k: str(v) for k, v in extra.items()})
    return env


def _run(cmd, **extra):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=_env(**extra), cwd=ROOT)


class World:
    pass


def _rec(sec, name, i):
    return gt.from_record(np.asarray(sec[name][96 * i:96 * i + 96]))


def _with(sec, name, edits):
    out = dict(sec)
    buf = bytearray(bytes(np.asarray(sec[name], np.uint8)))
    for i, (x, y) in edits.items():
        buf[96 * i:96 * i + 96] = bytes(gt.to_record(x, y))
    out[name] = bytes(buf)
    return out


def _swap(sec, name, i, j):
    a, b = _rec(sec, name, i), _rec(sec, name, j)
    assert a != b and a != (0, 0) and b != (0, 0), (name, i, j)
    return _with(sec, name, {i: b, j: a})


def _g2_copy(sec, dst, src):
    g2 = bytearray(bytes(np.asarray(sec["g2"], np.uint8)))
    assert g2[dst * 192:(dst + 1) * 192] != g2[src * 192:(src + 1) * 192]
    g2[dst * 192:(dst + 1) * 192] = g2[src * 192:(src + 1) * 192]
    out = dict(sec)
    out["g2"] = bytes(g2)
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import synth_circuit
    from tkmk import crs as crsmod
    w = World()
    w.tmp = str(tmp_path_factory.mktemp("crs_tables"))
    inst = synth_circuit.build(w.tmp, random.Random(83), s_max=8, n_gate_kinds=2, used_placements=8, bit_fraction=0.4)
    w.qap, w.synth, w.sp = inst["qap"], inst["synth"], inst["setup_params"]
    w.honest = os.path.join(w.tmp, "honest")
    os.makedirs(w.honest)
    r = _run([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", w.qap, "--output", w.honest])
    assert r.returncode == 0, r.stderr
    sp = w.sp
    s_max, m_i = sp["s_max"], sp["l_D"] - sp["l"]
    assert m_i >= 2
    w.points = {"gamma": sp["l"], "eta": m_i * s_max, "delta": (sp["m_D"] - sp["l_D"]) * s_max, "delta_small": 23, "alpha_chain": 4, "singles": 2}
    sec = dict(crsmod.read_payload(os.path.join(w.honest, "combined_sigma.tkcrs")))
    w.made = {}

    def stage(name, sections):
        d = os.path.join(w.tmp, name)
        os.makedirs(d)
        open(os.path.join(d, "combined_sigma.tkcrs"), "wb").write(crsmod.build_payload(sections))
        w.made[name] = d
    for c in ("rkyv", "tkcrs"):
        d = os.path.join(w.tmp, "only_" + c)
        os.makedirs(d)
        shutil.copy(os.path.join(w.honest, "combined_sigma." + c), d)
        w.made["only_" + c] = d
    eta, delta, gamma = "eta_inv_li_o_inter_alpha4_kj", "delta_inv_li_o_prv", "gamma_inv_o_inst"
    stage("eta_swap_across_j", _swap(sec, eta, 0 * s_max + 2, (m_i - 1) * s_max + 2))
    stage("eta_swap_within_j", _swap(sec, eta, (m_i - 1) * s_max + 1, (m_i - 1) * s_max + s_max - 1))
    live = [i for i in range(w.points["delta"]) if _rec(sec, delta, i) != (0, 0)]           # tables may hold infinity
    at = live[len(live) // 2]
    stage("delta_doubled", _with(sec, delta, {at: gt.mul(2, _rec(sec, delta, at))}))
    at = max(i for i in range(sp["l"] - 1) if (0, 0) not in (_rec(sec, gamma, i), _rec(sec, gamma, i + 1)) and _rec(sec, gamma, i) != _rec(sec, gamma, i + 1))
    stage("gamma_is_its_neighbour", _with(sec, gamma, {at: _rec(sec, gamma, at + 1)}))
    stage("xh_0_1_swapped", _swap(sec, "delta_inv_alphak_xh_tx", 0, 1))
    stage("yi_0_3_swapped", _swap(sec, "delta_inv_alphak_yi_ty", 0, 3))
    stage("g2_gamma_is_delta", _g2_copy(sec, 5, 6))
    stage("g2_alpha2_is_alpha", _g2_copy(sec, 2, 1))
    stage("singles_eta_is_delta", _with(sec, "g1", {4: _rec(sec, "g1", 3)}))
    return w


def _check_bin(world, crs, lib=None, **env):
    r = _run([os.path.join(BIN, "crs-check"), "--crs", crs, "--subcircuit-library", lib or world.qap, "--circuit"], **env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()[-1], r.stderr


@pytest.mark.parametrize("container", ["rkyv", "tkcrs"])
def test_honest_crs_passes_the_table_checks_from_both_containers(gpu, world, container):
    from tkmk import verify
    crs = world.made["only_" + container]
    ok, rep = verify.crs_audit(world.qap, crs, circuit=True)
    assert ok is True and rep["ok"] is True and rep["reason"] == "" and rep["circuit"] is True
    assert [t["name"] for t in rep["tables"]] == TABLES
    assert all(t["ok"] is True for t in rep["tables"]), rep["tables"]
    assert {t["name"]: t["points"] for t in rep["tables"]} == world.points
    assert set(rep["table_seconds"]) == {"library", "grids", "msm", "pairings"}
    ok0, rep0 = verify.crs_audit(world.qap, crs)                           # without the flag: the old report, the new keys null
    assert ok0 is True and rep0["tables"] is None and rep0["circuit"] is None and rep0["table_seconds"] is None
    assert [json.dumps(rep0[k]) for k in OLD_KEYS] == [json.dumps(rep[k]) for k in OLD_KEYS]
    assert set(rep0["seconds"]) == set(rep["seconds"]) == {"upload", "membership", "g2", "msm", "pairings", "total"}
    assert list(rep0)[:8] == OLD_KEYS + ["seconds"]
    last, err = _check_bin(world, crs)
    assert last == "true" and "combined_sigma." + container in err
    for t in TABLES:
        assert "table %s " % t in err, err


def test_crs_made_under_generator_7_passes_in_a_process_with_nothing_set(gpu, world):
    out = os.path.join(world.tmp, "honest_gen7")
    os.makedirs(out)
    r = _run([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", world.qap, "--output", out, "--format", "tkcrs"],
             TKMK_FR_ROOT_GENERATOR=7)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(out, "combined_sigma.tkcrs"), "rb").read() != open(os.path.join(world.honest, "combined_sigma.tkcrs"), "rb").read()
    last, err = _check_bin(world, out)
    assert last == "true", err


# name -> (tables that must be false, tables that may be false as well)
TAMPERS = {"eta_swap_across_j": ({"eta"}, set()),
           "eta_swap_within_j": ({"eta"}, set()),
           "delta_doubled": ({"delta"}, set()),
           "gamma_is_its_neighbour": ({"gamma"}, set()),
           "xh_0_1_swapped": ({"delta_small"}, set()),
           "yi_0_3_swapped": (set(), {"delta_small", "alpha_chain"}),                  # caught by either, at least one
           "g2_gamma_is_delta": ({"gamma"}, set()),
           # every equation with an alpha^2 term on its right side sees this one; the chain (alpha and H only) and the singles do not
           "g2_alpha2_is_alpha": ({"delta_small"}, {"gamma", "eta", "delta"}),
           "singles_eta_is_delta": ({"singles"}, set())}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", sorted(TAMPERS))
def test_table_tampers_are_refused_and_named_under_every_seed(gpu, world, monkeypatch, name, seed):
    from tkmk import verify
    must, may = TAMPERS[name]
    monkeypatch.setenv("TKMK_CRS_AUDIT_SEED", str(seed))
    ok, rep = verify.crs_audit(world.qap, world.made[name], testing=True, circuit=True)
    assert ok is False and rep["ok"] is False and rep["circuit"] is False
    for s in rep["sections"]:                                               # every point is valid, xy_powers untouched
        assert (s["noncanonical"], s["off_curve"], s["not_in_subgroup"]) == (0, 0, 0)
    assert (rep["g2"], rep["anchors"], rep["ratio_y"], rep["ratio_x"]) == (True, True, True, True)
    failed = {t["name"] for t in rep["tables"] if not t["ok"]}
    assert [t["name"] for t in rep["tables"]] == TABLES
    assert failed and must <= failed <= must | may, failed
    first = next(t["name"] for t in rep["tables"] if not t["ok"])
    assert "table %s:" % first in rep["reason"], rep["reason"]
    ok, rep = verify.crs_audit(world.qap, world.made[name], testing=True)  # the gap the feature closes: without it, still true
    assert ok is True and rep["tables"] is None
    ok, rep = verify.crs_audit(world.qap, world.made["only_tkcrs"], testing=True, circuit=True)   # the honest CRS under the same seed
    assert ok is True and all(t["ok"] for t in rep["tables"])


def test_binary_refuses_a_table_tamper_and_names_the_table(gpu, world):
    last, err = _check_bin(world, world.made["eta_swap_across_j"])
    assert last == "false" and "table eta:" in err and "eta_inv_li_o_inter_alpha4_kj" in err and "FAILED" in err


def test_crs_of_another_circuit_of_the_same_shape_is_refused(gpu, world):
    import synth_circuit
    other = os.path.join(world.tmp, "other_circuit")
    os.makedirs(other)
    inst = synth_circuit.build(other, random.Random(84), s_max=8, n_gate_kinds=2, used_placements=8, bit_fraction=0.4)
    if inst["setup_params"] != world.sp:
        pytest.skip("the second synthetic circuit has another shape: %r != %r" % (inst["setup_params"], world.sp))
    from tkmk import verify
    ok, rep = verify.crs_audit(inst["qap"], world.made["only_tkcrs"], circuit=True)
    assert ok is False and rep["circuit"] is False and rep["ratio_x"] is True
    failed = [t["name"] for t in rep["tables"] if not t["ok"]]
    assert failed and set(failed) <= {"gamma", "eta", "delta"} and "table %s:" % failed[0] in rep["reason"]
    assert verify.crs_audit(inst["qap"], world.made["only_tkcrs"])[0] is True


def test_library_without_the_circuit_files_is_an_error_not_a_verdict(gpu, world):
    from tkmk import service, verify
    bare = os.path.join(world.tmp, "bare_library")
    os.makedirs(bare)
    shutil.copy(os.path.join(world.qap, "setupParams.json"), bare)
    assert verify.crs_audit(bare, world.made["only_tkcrs"])[0] is True      # the audit without the circuit needs nothing else
    with pytest.raises(service.ProverError):
        verify.crs_audit(bare, world.made["only_tkcrs"], circuit=True)
    r = _run([os.path.join(BIN, "crs-check"), "--crs", world.made["only_tkcrs"], "--subcircuit-library", bare, "--circuit"])
    assert r.returncode == 1 and "true" not in r.stdout and "false" not in r.stdout and "subcircuitInfo.json" in r.stderr


OPEN_CODE = """
import json, os, random, sys
import tkmk
from tkmk import service
from tkmk.prove import random_mixer
qap, synth, tmp, honest, swapped = sys.argv[1:6]
tkmk.set_device(0)
hx = lambda v: [hx(e) for e in v] if isinstance(v, list) else "0x%x" % v
mixer = os.path.join(tmp, "mixer_tables_%d.json" % os.getpid())
json.dump({k: hx(v) for k, v in random_mixer(random.Random(7)).items()}, open(mixer, "w"))
out = {}
with service.Prover(qap, honest, testing=True) as p:
    out["proof"] = p.prove(synth, None, testing_mixer_json=mixer)[0]
try:
    with service.Prover(qap, swapped, testing=True) as p:
        out["swapped"] = "opened"
except service.ProverError as e:
    out["swapped"] = [e.code, str(e)]
print(json.dumps(out))
"""


def _open(world, **env):
    r = _run([sys.executable, "-c", OPEN_CODE, world.qap, world.synth, world.tmp, world.made["only_tkcrs"], world.made["eta_swap_across_j"]], **env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_open_refuses_a_table_tamper_only_under_the_full_audit(gpu, world):
    plain = _open(world)
    basic = _open(world, TKMK_PROVER_CHECK_CRS=1)
    full = _open(world, TKMK_PROVER_CHECK_CRS=2)
    assert plain["proof"] and basic["proof"] == plain["proof"] == full["proof"]        # byte-equal under fixed blinding
    code, msg = full["swapped"]
    assert code == 11 and "table eta:" in msg and "audit" in msg, msg
    assert plain["swapped"] == "opened" and basic["swapped"] == "opened"
