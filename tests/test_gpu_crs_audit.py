"""gpu tier: the audit of a reference string (host/tkmk_crs_audit.hpp: tkmk_crs_audit_files, bin/crs-check, TKMK_PROVER_CHECK_CRS=1 at
tkmk_prover_open).  One small circuit and one `trusted-setup --fixed-tau`, as tests/test_gpu_crs_root_identify.py; every tampered copy
is the flat payload rewritten with tkmk.crs.read_payload / build_payload.  Membership tampers put ONE bad record into a table (the
section, index and reason must be named); structure tampers keep every point valid, so only the ratio check can see them, and are run
under three seeds through the testing library.  The prover's opens run in child processes."""
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
    """a copy of the sections with records of one section replaced: edits = {index: (x, y)}"""
    out = dict(sec)
    buf = bytearray(bytes(np.asarray(sec[name], np.uint8)))
    for i, (x, y) in edits.items():
        buf[96 * i:96 * i + 96] = bytes(gt.to_record(x, y))
    out[name] = bytes(buf)
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import synth_circuit
    from tkmk import crs as crsmod
    w = World()
    w.tmp = str(tmp_path_factory.mktemp("crs_audit"))
    inst = synth_circuit.build(w.tmp, random.Random(83), s_max=8, n_gate_kinds=2, used_placements=8, bit_fraction=0.4)
    w.qap, w.synth, w.sp = inst["qap"], inst["synth"], inst["setup_params"]
    w.honest = os.path.join(w.tmp, "honest")
    os.makedirs(w.honest)
    r = _run([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", w.qap, "--output", w.honest])
    assert r.returncode == 0, r.stderr
    sp = w.sp
    w.m_i = sp["l_D"] - sp["l"]
    w.rs_x, w.rs_y = max(2 * sp["n"], 2 * w.m_i), 2 * sp["s_max"]
    w.sizes = {"xy_powers": w.rs_x * w.rs_y, "gamma_inv_o_inst": sp["l"], "eta_inv_li_o_inter_alpha4_kj": w.m_i * sp["s_max"],
               "delta_inv_li_o_prv": (sp["m_D"] - sp["l_D"]) * sp["s_max"], "delta_inv_alphak_xh_tx": 9, "delta_inv_alpha4_xj_tx": 2,
               "delta_inv_alphak_yi_ty": 12, "g1_singles": 6}
    sec = dict(crsmod.read_payload(os.path.join(w.honest, "combined_sigma.tkcrs")))
    w.sec = sec
    w.made = {}

    def stage(name, sections):
        d = os.path.join(w.tmp, name)
        os.makedirs(d)
        open(os.path.join(d, "combined_sigma.tkcrs"), "wb").write(crsmod.build_payload(sections))
        w.made[name] = d
        return d
    for c in ("rkyv", "tkcrs"):
        d = os.path.join(w.tmp, "only_" + c)
        os.makedirs(d)
        shutil.copy(os.path.join(w.honest, "combined_sigma." + c), d)
        w.made["only_" + c] = d
    rs_y = w.rs_y
    # membership: one bad record each
    w.deep = (w.rs_x // 2) * rs_y + rs_y // 2 + 1
    stage("xy_torsion", _with(sec, "xy_powers", {w.deep: gt.add(_rec(sec, "xy_powers", w.deep), (0, 2))}))
    w.delta_at = w.sizes["delta_inv_li_o_prv"] // 2
    x, y = _rec(sec, "delta_inv_li_o_prv", w.delta_at)
    stage("delta_off_curve", _with(sec, "delta_inv_li_o_prv", {w.delta_at: (x, (y + 1) % gt.P)}))
    w.gamma_at = max(i for i in range(w.sizes["gamma_inv_o_inst"]) if _rec(sec, "gamma_inv_o_inst", i) != (0, 0))   # tables may hold infinity
    x, y = _rec(sec, "gamma_inv_o_inst", w.gamma_at)
    stage("gamma_plus_p", _with(sec, "gamma_inv_o_inst", {w.gamma_at: (x, y + gt.P)}))
    stage("xy_zeroed", _with(sec, "xy_powers", {w.deep: (0, 0)}))
    # structure: valid points in the wrong place — outside the m_I x s_max corner the root-of-unity check of open reads, so that open
    # without the audit still takes them
    a, b1, b2 = min(3, w.rs_x - 1), sp["s_max"] + 5, sp["s_max"] + 6
    i1, i2 = a * rs_y + b1, a * rs_y + b2
    stage("row_swap", _with(sec, "xy_powers", {i1: _rec(sec, "xy_powers", i2), i2: _rec(sec, "xy_powers", i1)}))
    a1, a2, b = w.rs_x - 1, w.rs_x - 2, sp["s_max"] + 3
    j1, j2 = a1 * rs_y + b, a2 * rs_y + b
    stage("col_swap", _with(sec, "xy_powers", {j1: _rec(sec, "xy_powers", j2), j2: _rec(sec, "xy_powers", j1)}))
    stage("doubled", _with(sec, "xy_powers", {w.deep: gt.mul(2, _rec(sec, "xy_powers", w.deep))}))
    g2 = bytearray(bytes(np.asarray(sec["g2"], np.uint8)))
    g2[9 * 192:10 * 192] = g2[8 * 192:9 * 192]                              # sigma_2.y := sigma_2.x
    swapped = dict(sec)
    swapped["g2"] = bytes(g2)
    stage("g2_y_is_x", swapped)
    return w


def _check_bin(world, crs):
    r = _run([os.path.join(BIN, "crs-check"), "--crs", crs, "--subcircuit-library", world.qap])
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()[-1], r.stderr


@pytest.mark.parametrize("container", ["rkyv", "tkcrs"])
def test_honest_crs_passes_from_both_containers(gpu, world, container):
    from tkmk import verify
    crs = world.made["only_" + container]
    assert os.listdir(crs) == ["combined_sigma." + container]
    ok, rep = verify.crs_audit(world.qap, crs)
    assert ok is True and rep["ok"] is True and rep["reason"] == ""
    assert (rep["g2"], rep["anchors"], rep["ratio_y"], rep["ratio_x"]) == (True, True, True, True)
    assert {s["name"]: s["points"] for s in rep["sections"]} == world.sizes
    for s in rep["sections"]:
        assert (s["noncanonical"], s["off_curve"], s["not_in_subgroup"], s["first_bad"]) == (0, 0, 0, None), s
    assert rep["sections"][0]["name"] == "xy_powers" and rep["sections"][0]["infinity"] == 0
    assert set(rep["seconds"]) == {"upload", "membership", "g2", "msm", "pairings", "total"}
    last, err = _check_bin(world, crs)
    assert last == "true" and "combined_sigma." + container in err and "xy_powers" in err


def test_crs_check_usage_and_unreadable_input(gpu, world):
    empty = os.path.join(world.tmp, "empty")
    os.makedirs(empty, exist_ok=True)
    r = _run([os.path.join(BIN, "crs-check"), "--crs", empty, "--subcircuit-library", world.qap])
    assert r.returncode == 1 and "true" not in r.stdout and "false" not in r.stdout and "combined_sigma" in r.stderr
    assert _run([os.path.join(BIN, "crs-check")]).returncode == 2
    from tkmk import service, verify
    with pytest.raises(service.ProverError):
        verify.crs_audit(world.qap, empty)


MEMBERSHIP = [("xy_torsion", "xy_powers", "deep", "not_in_subgroup", "subgroup"),
              ("delta_off_curve", "delta_inv_li_o_prv", "delta_at", "off_curve", "not on the curve"),
              ("gamma_plus_p", "gamma_inv_o_inst", "gamma_at", "noncanonical", "not reduced"),
              ("xy_zeroed", "xy_powers", "deep", "infinity", "infinity")]


@pytest.mark.parametrize("name,section,at,counter,words", MEMBERSHIP)
def test_membership_tampers_are_named(gpu, world, name, section, at, counter, words):
    from tkmk import verify
    index = getattr(world, at)
    ok, rep = verify.crs_audit(world.qap, world.made[name])
    assert ok is False and rep["ok"] is False
    assert "%s[%d]" % (section, index) in rep["reason"] and words in rep["reason"], rep["reason"]
    by_name = {s["name"]: s for s in rep["sections"]}
    assert by_name[section][counter] == 1
    if counter != "infinity":
        assert by_name[section]["first_bad"] == index
    for s in rep["sections"]:                                               # nothing else is reported
        bad = s["noncanonical"] + s["off_curve"] + s["not_in_subgroup"]
        assert bad == (1 if s["name"] == section and counter != "infinity" else 0), s
    assert (rep["ratio_y"], rep["ratio_x"]) == (None, None)                 # an MSM over such a table proves nothing: not run
    last, err = _check_bin(world, world.made[name])
    assert last == "false" and "%s[%d]" % (section, index) in err


STRUCTURE = [("row_swap", "ratio_y"), ("col_swap", "ratio_x"), ("doubled", None), ("g2_y_is_x", "ratio_y")]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name,flag", STRUCTURE)
def test_structure_tampers_are_refused_under_every_seed(gpu, world, monkeypatch, name, flag, seed):
    from tkmk import verify
    monkeypatch.setenv("TKMK_CRS_AUDIT_SEED", str(seed))
    ok, rep = verify.crs_audit(world.qap, world.made[name], testing=True)
    assert ok is False and rep["ok"] is False and "xy_powers" in rep["reason"]
    for s in rep["sections"]:                                               # every point is valid: membership sees nothing
        assert (s["noncanonical"], s["off_curve"], s["not_in_subgroup"]) == (0, 0, 0)
    assert rep["g2"] is True and rep["anchors"] is True
    if flag:
        assert rep[flag] is False
    assert rep["ratio_y"] is False or rep["ratio_x"] is False
    ok, rep = verify.crs_audit(world.qap, world.made["only_tkcrs"], testing=True)   # the honest CRS under the same seed
    assert ok is True and rep["ratio_y"] is True and rep["ratio_x"] is True


def test_structure_tamper_through_the_production_library_and_binary(gpu, world):
    from tkmk import verify
    ok, rep = verify.crs_audit(world.qap, world.made["row_swap"])
    assert ok is False and rep["ratio_y"] is False
    last, err = _check_bin(world, world.made["row_swap"])
    assert last == "false" and "along Y" in err


OPEN_CODE = """
import json, os, random, sys
import tkmk
from tkmk import service
from tkmk.prove import random_mixer
qap, synth, tmp, honest, swapped = sys.argv[1:6]
tkmk.set_device(0)
hx = lambda v: [hx(e) for e in v] if isinstance(v, list) else "0x%x" % v
mixer = os.path.join(tmp, "mixer_audit_%d.json" % os.getpid())
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
    r = _run([sys.executable, "-c", OPEN_CODE, world.qap, world.synth, world.tmp, world.made["only_tkcrs"], world.made["row_swap"]], **env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_open_with_and_without_the_knob(gpu, world):
    plain = _open(world)
    checked = _open(world, TKMK_PROVER_CHECK_CRS=1)
    zero = _open(world, TKMK_PROVER_CHECK_CRS=0)
    assert plain["proof"] and checked["proof"] == plain["proof"] == zero["proof"]      # byte-equal under fixed blinding
    code, msg = checked["swapped"]
    assert code == 11 and "xy_powers" in msg and "audit" in msg, msg
    assert plain["swapped"] == "opened" and zero["swapped"] == "opened"                 # the gap the knob closes; unchanged without it
