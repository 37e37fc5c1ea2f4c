"""CPU tier: the native verifier — tokamak-zk-evm_amd/bin/verify (host/verify_main.cpp) and tkmk_verify_files (include/tkmk_prover.h,
tkmk/verify.py), both over host/tkmk_verify.hpp — on the files of one small proof made by the restated prover of tests/prove_ref.py, in
the shape of tests/test_pairing_ref.py::test_verify_snark_with_pairings (s_max = 8, m_I > 2: the two root-of-unity generators really
differ).  The honest proof verifies; every tampered input gives `false` with exit status 0 and a reason; an unreadable input is an error
that names the file; the verdict equals the Python verifier's (tests/prove_ref.py verify_snark_pairing: 10 Python pairings per call, two
calls); the binary links neither the device library nor the ROCm runtime."""
import copy
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "tokamak-zk-evm_amd", "bin")
VERIFY = os.path.join(BIN, "verify")
PINS = json.load(open(os.path.join(HERE, "golden", "pins.json")))
G2_NAMES = ("H", "alpha", "alpha2", "alpha3", "alpha4", "gamma", "delta", "eta", "x", "y")


class World:
    pass


def _g1_json(rec):
    b = bytes(np.asarray(rec, np.uint8))
    return {"x": "0x" + b[:48][::-1].hex(), "y": "0x" + b[48:][::-1].hex()}


def _g2_json(pt):
    """one big-endian hex number per coordinate over the 96-byte Fp2 element, imaginary part in the high half (G2serde)"""
    if pt is None:
        return {"x": "0x" + "00" * 96, "y": "0x" + "00" * 96}
    return {"x": "0x%0192x" % ((pt[0][1] << 384) | pt[0][0]), "y": "0x%0192x" % ((pt[1][1] << 384) | pt[1][0])}


def _sigma_verify_doc(crs_g1, sigma2):
    return {"G": _g1_json(crs_g1["G"]), "H": _g2_json(sigma2["H"]), "sigma_1": {"x": _g1_json(crs_g1["x"]), "y": _g1_json(crs_g1["y"])},
            "sigma_2": {k: _g2_json(sigma2[k]) for k in G2_NAMES[1:]}, "lagrange_KL": _g1_json(crs_g1["lagrange_KL"])}


@pytest.fixture(scope="module")
def world(oracle, tkmk, tmp_path_factory):
    import prove_ref
    import synth_circuit
    from tkmk import g2, proofio
    from tkmk.prove import random_mixer
    w = World()
    w.tmp = tmp_path_factory.mktemp("verify_native")
    w.R = oracle.R_MOD
    g = oracle.to_bytes([int(PINS["fixed_tau_g1_x"], 16), int(PINS["fixed_tau_g1_y"], 16)], 48)
    h = g2.from_hex_pair(PINS["fixed_tau_g2_x"], PINS["fixed_tau_g2_y"])
    inst = synth_circuit.build(str(w.tmp), random.Random(17), s_max=8, n_gate_kinds=2, used_placements=7)
    w.sp, w.qap, w.synth, w.instance = inst["setup_params"], inst["qap"], inst["synth"], inst["instance"]
    assert w.sp["l_D"] - w.sp["l"] > 2
    w.tau = {k: int(PINS["tau_" + k], 16) for k in ("x", "y", "alpha", "gamma", "delta", "eta")}
    crs = prove_ref.sigma_gen(inst, w.tau)
    d, s, ch, p4t, rp = prove_ref.run(inst, crs, random_mixer(random.Random(17)), g)
    pre = prove_ref.preprocess(rp, inst, crs)
    w.rec = lambda dlog: np.asarray(prove_ref.g1_of(dlog, g))                          # noqa: E731
    w.dlog = d
    w.points = {k: w.rec(v) for k, v in d.items()}
    w.scalars = dict(s)
    w.crs_g1 = {"G": w.rec(1), "x": w.rec(crs["tau_x"]), "y": w.rec(crs["tau_y"]), "lagrange_KL": w.rec(crs["lagrange_KL"])}
    w.pre_points = {k: w.rec(v) for k, v in pre.items()}
    w.h = h
    w.sigma2 = dict(zip(G2_NAMES, g2.sigma2_gen(w.tau, h)))
    w.proofio, w.g2 = proofio, g2
    w.honest = _case(w, "honest")
    return w


def _case(w, name, points=None, scalars=None, pre_points=None, sigma2=None, instance=None, crs_g1=None, proof_doc=None, preprocess_doc=None):
    """<tmp>/<name>/{crs, synth, pre, proof}: the honest files with the given parts replaced -> the argv tokamak-cli sends"""
    d = w.tmp / name
    for sub in ("crs", "synth", "pre", "proof"):
        (d / sub).mkdir(parents=True)
    json.dump(_sigma_verify_doc(crs_g1 or w.crs_g1, sigma2 or w.sigma2), open(d / "crs" / "sigma_verify.json", "w"), indent=2)
    json.dump(instance or w.instance, open(d / "synth" / "instance.json", "w"))
    w.proofio.write_json(d / "pre" / "preprocess.json", preprocess_doc or w.proofio.format_preprocess(pre_points or w.pre_points))
    w.proofio.write_json(d / "proof" / "proof.json", proof_doc or w.proofio.format_proof(points or w.points, scalars or w.scalars))
    return {"crs": str(d / "crs"), "synth": str(d / "synth"), "pre": str(d / "pre"), "proof": str(d / "proof")}


def _argv(c):
    return ["--crs", c["crs"], "--synthesizer-stat", c["synth"], "--preprocess", c["pre"], "--proof", c["proof"]]      # cli.ts backendVerifyArgs


def _run(argv, env_extra=None, drop=("TKMK_SUBCIRCUIT_LIBRARY", "XDG_CACHE_HOME"), home=None):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    if home is not None:
        env["HOME"] = str(home)
    env.update(env_extra or {})
    return subprocess.run([VERIFY] + argv, capture_output=True, text=True, timeout=60, env=env)


def _both(w, c, root_generator=0):
    """bin/verify under the CLI's argv and tkmk_verify_files on the same directories -> (verdict, stderr of the binary, report)"""
    from tkmk import verify
    env = {"TKMK_SUBCIRCUIT_LIBRARY": w.qap}
    if root_generator:
        env["TKMK_FR_ROOT_GENERATOR"] = str(root_generator)
    r = _run(_argv(c), env)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.strip().split("\n")
    assert lines[-3:-1] == ["Verifier initialization...", "Verifying the proof..."] and lines[-1] in ("true", "false"), r.stdout
    ok, rep = verify.verify_files(w.qap, c["crs"], c["synth"], c["pre"], c["proof"], root_generator=root_generator)
    assert ok == (lines[-1] == "true") and rep["ok"] == ok
    if not ok:
        assert rep["reason"] and rep["reason"] in r.stderr, (rep, r.stderr)
    return ok, r.stderr, rep


def test_honest_proof_verifies_by_both_routes(world):
    import prove_ref
    import pyref
    from tkmk.transcript import TranscriptManager
    w = world
    ok, err, rep = _both(w, w.honest)
    assert ok and rep["reason"] == ""
    assert rep["generator"] == pyref.root_generator() and ("root-of-unity generator %d" % rep["generator"]) in err
    m = TranscriptManager()                                                    # Verifier::collect_challenges
    m.add_proof0(*(w.points[k] for k in ("U", "V", "W", "Q_AX", "Q_AY", "B")))
    thetas = m.get_thetas()
    m.add_proof1(w.points["R"])
    kappa0 = m.get_kappa0()
    m.add_proof2(w.points["Q_CX"], w.points["Q_CY"])
    chi, zeta = m.get_chi_zeta()
    m.add_proof3(*(w.scalars[k] for k in ("V_eval", "R_eval", "R_omegaX_eval", "R_omegaX_omegaY_eval")))
    kappa1 = m.get_kappa1()
    assert [int(t, 16) for t in rep["thetas"]] == list(thetas)
    assert [int(rep[k], 16) for k in ("kappa0", "chi", "zeta", "kappa1")] == [kappa0, chi, zeta, kappa1]
    sp = w.sp
    a = [int(v, 16) for v in w.instance["a_pub_user"][:sp["l_user"]]] + [int(v, 16) for v in w.instance["a_pub_block"][:sp["l_free"] - sp["l_user"]]]
    assert int(rep["a_eval"], 16) == prove_ref.interpolate([[v] for v in a], sp["l_free"], 1).eval(chi, zeta)
    # kappa2 is fresh every time: the verdict does not depend on it
    assert all(_both(w, w.honest)[0] for _ in range(2))


def _expect_false(w, c, reason_part, **kw):
    ok, err, rep = _both(w, c, **kw)
    assert not ok and reason_part in rep["reason"], rep
    return rep


def test_tampered_proof_points_and_evaluations(world, oracle):
    w = world
    bad = dict(w.points, Pi_X=np.asarray(oracle.g1_add(w.points["Pi_X"].copy(), w.crs_g1["G"].copy())))      # Pi_X + G
    _expect_false(w, _case(w, "pi_x", points=bad), "pairing product != 1")
    _expect_false(w, _case(w, "r_eval", scalars=dict(w.scalars, R_eval=(w.scalars["R_eval"] + 1) % w.R)), "pairing product != 1")
    pre = dict(w.pre_points, s0=w.pre_points["s1"], s1=w.pre_points["s0"])
    _expect_false(w, _case(w, "s0_s1", pre_points=pre), "pairing product != 1")


def test_tampered_public_input(world):
    w = world
    ins = copy.deepcopy(w.instance)
    assert w.sp["l_user"] > 0
    ins["a_pub_user"][0] = hex((int(ins["a_pub_user"][0], 16) + 1) % w.R)
    rep = _expect_false(w, _case(w, "public_input", instance=ins), "pairing product != 1")
    assert rep["a_eval"] != _both(w, w.honest)[2]["a_eval"] and rep["chi"] == _both(w, w.honest)[2]["chi"]


def test_tampered_reference_string(world):
    w = world
    wrong = dict(w.sigma2, delta=w.g2.scalar_mul(w.tau["delta"] + 1, w.h))
    _expect_false(w, _case(w, "delta", sigma2=wrong), "pairing product != 1")
    rep = _expect_false(w, _case(w, "no_sigma2", sigma2={k: None for k in G2_NAMES}), "holds no Sigma2")
    assert "thetas" not in rep                                                   # refused before any transcript work
    _expect_false(w, _case(w, "no_alpha", sigma2=dict(w.sigma2, alpha=None)), "sigma_2.alpha is the point at infinity")


def test_invalid_group_elements_give_false_not_an_error(world, oracle):
    w, P = world, oracle.P_MOD
    rec = lambda x, y: np.frombuffer(int(x).to_bytes(48, "little") + int(y).to_bytes(48, "little"), np.uint8).copy()     # noqa: E731
    x, y = oracle.to_ints(w.points["Q_AY"], 48)
    _expect_false(w, _case(w, "off_curve", points=dict(w.points, Q_AY=rec(x, (y + 1) % P))), "proof.json: Q_AY is not on the curve")
    sx = next(v for v in range(1, 100) if pow((v ** 3 + 4) % P, (P - 1) // 2, P) == 1)
    stray = rec(sx, pow((sx ** 3 + 4) % P, (P + 1) // 4, P))
    assert oracle.g1_on_curve(stray)
    _expect_false(w, _case(w, "cofactor", pre_points=dict(w.pre_points, O_pub_fix=stray)), "preprocess.json: O_pub_fix is not in the subgroup")
    # a coordinate >= p: representable in the document, refused by the range check
    doc = w.proofio.format_proof(w.points, w.scalars)
    be = int(x + P).to_bytes(48, "big")
    i = 2 * w.proofio.PROOF_POINT_ORDER.index("Q_AY")
    doc["proof_entries_part1"][i], doc["proof_entries_part2"][i] = "0x" + be[:16].hex(), "0x" + be[16:].hex()
    _expect_false(w, _case(w, "not_reduced", proof_doc=doc), "proof.json: Q_AY has a coordinate that is not reduced")
    crs_g1 = dict(w.crs_g1, lagrange_KL=rec(*[(v + 1) % P for v in oracle.to_ints(w.crs_g1["lagrange_KL"], 48)]))
    _expect_false(w, _case(w, "kl", crs_g1=crs_g1), "sigma_verify.json: lagrange_KL is not on the curve")


def test_the_generator_is_an_input_and_never_guessed(world):
    """files made under one generator, the verifier pinned to the other: false — by the environment for the binary, by the argument for
    the call; the report names the generator used"""
    import pyref
    w = world
    made_under = pyref.root_generator()
    other = 7 if made_under != 7 else 5
    rep = _expect_false(w, w.honest, "pairing product != 1", root_generator=other)
    assert rep["generator"] == other
    ok, _, rep = _both(w, w.honest, root_generator=made_under)
    assert ok and rep["generator"] == made_under


def test_verdict_equals_the_python_verifier(world):
    """honest and one tampered case through tests/prove_ref.py verify_snark_pairing on the same points (20 Python pairings)"""
    import prove_ref
    from tkmk.transcript import TranscriptManager
    w = world
    bad_points = dict(w.points, M_Y=w.rec(w.dlog["M_Y"] + 1))
    for name, points, want in (("py_honest", w.points, True), ("py_m_y", bad_points, False)):
        m = TranscriptManager()
        m.add_proof0(*(points[k] for k in ("U", "V", "W", "Q_AX", "Q_AY", "B")))
        th = m.get_thetas()
        m.add_proof1(points["R"])
        k0 = m.get_kappa0()
        m.add_proof2(points["Q_CX"], points["Q_CY"])
        chi, zeta = m.get_chi_zeta()
        m.add_proof3(*(w.scalars[k] for k in ("V_eval", "R_eval", "R_omegaX_eval", "R_omegaX_omegaY_eval")))
        ch = {"thetas": th, "kappa0": k0, "chi": chi, "zeta": zeta, "kappa1": m.get_kappa1()}
        native, _, rep = _both(w, w.honest if points is w.points else _case(w, name, points=points))
        python = bool(prove_ref.verify_snark_pairing(points, w.scalars, ch, w.sp, w.crs_g1, w.pre_points, w.sigma2, int(rep["a_eval"], 16),
                                                     random.Random(5).randrange(1, w.R)))
        assert native == python == want, name


def test_unreadable_inputs_are_errors_that_name_the_file(world):
    from tkmk import service, verify
    w = world

    def both_fail(c, *parts):
        r = _run(_argv(c), {"TKMK_SUBCIRCUIT_LIBRARY": w.qap})
        assert r.returncode == 1 and r.stdout.strip().split("\n")[-1] not in ("true", "false"), (r.stdout, r.stderr)
        with pytest.raises(service.ProverError) as e:
            verify.verify_files(w.qap, c["crs"], c["synth"], c["pre"], c["proof"])
        for p in parts:
            assert p in r.stderr and p in str(e.value), (p, r.stderr, str(e.value))

    c = _case(w, "missing_proof")
    os.remove(os.path.join(c["proof"], "proof.json"))
    both_fail(c, "No proof is found. Run the Prove first.", "proof.json")
    c = _case(w, "missing_sigma")
    os.remove(os.path.join(c["crs"], "sigma_verify.json"))
    both_fail(c, "No reference string is found. Run the Setup first (expected sigma_verify.json).")
    c = _case(w, "missing_pre")
    os.remove(os.path.join(c["pre"], "preprocess.json"))
    both_fail(c, "No Verifier preprocess is found. Run the Preprocess first.", "preprocess.json")
    doc = w.proofio.format_proof(w.points, w.scalars)
    doc["proof_entries_part2"][3] = doc["proof_entries_part2"][3][:-3]            # a truncated hex string
    both_fail(_case(w, "truncated", proof_doc=doc), "proof.json", "Invalid format")
    doc = w.proofio.format_proof(w.points, w.scalars)
    doc["proof_entries_part1"].pop()                                              # a part list one entry short
    both_fail(_case(w, "short", proof_doc=doc), "proof.json", "unexpected proof entry count")
    doc = w.proofio.format_preprocess(w.pre_points)
    doc["preprocess_entries_part2"].pop()
    both_fail(_case(w, "short_pre", preprocess_doc=doc), "preprocess.json", "unexpected preprocess entry count")
    c = _case(w, "bad_hex")
    sv = json.load(open(os.path.join(c["crs"], "sigma_verify.json")))
    sv["sigma_1"]["x"]["y"] = "0xzz"
    json.dump(sv, open(os.path.join(c["crs"], "sigma_verify.json"), "w"))
    both_fail(c, "sigma_verify.json", "invalid hex digit")
    del sv["sigma_2"]["eta"]
    sv["sigma_1"]["x"]["y"] = "0x01"
    json.dump(sv, open(os.path.join(c["crs"], "sigma_verify.json"), "w"))
    both_fail(c, "sigma_verify.json", "missing field 'eta'")
    c = _case(w, "no_instance")
    open(os.path.join(c["synth"], "instance.json"), "w").write('{"a_pub_user": []')
    both_fail(c, "instance.json")


def test_binary_is_host_only():
    r = subprocess.run(["ldd", VERIFY], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "libtkmk_hip" not in r.stdout and "libamdhip64" not in r.stdout and "libhsa" not in r.stdout, r.stdout


def test_argv_forms_and_library_resolution(world, tmp_path):
    """what tests/test_cli_argv.py covers for the other three binaries: `--flag=value`, a missing library with the reason, the library
    of the installation, usage errors with clap's exit status, --help / --version"""
    import re
    w, c = world, world.honest
    r = _run(["--proof=" + c["proof"], "--subcircuit-library=" + w.qap, "--crs", c["crs"], "--preprocess=" + c["pre"], "--synthesizer-stat", c["synth"]])
    assert r.returncode == 0 and r.stdout.strip().endswith("\ntrue") and ("Subcircuit library: " + os.path.realpath(w.qap)) in r.stdout, (r.stdout, r.stderr)
    # the CLI's argv with no library anywhere: the reason, exit status 1, no usage text
    r = _run(_argv(c), home=tmp_path / "home")
    assert r.returncode == 1 and "--subcircuit-library is required" in r.stderr and "TKMK_SUBCIRCUIT_LIBRARY" in r.stderr and "Usage" not in r.stderr
    r = _run(_argv(c), {"TKMK_SUBCIRCUIT_LIBRARY": str(tmp_path / "nowhere")}, home=tmp_path / "home")
    assert r.returncode == 1 and "holds no setupParams.json" in r.stderr
    # the cache directory of a reference release binary, and tokamak-cli's runtime layout <runtime>/bin + <runtime>/resource
    snap = tmp_path / "xdg" / "tokamak-zk-evm" / "subcircuit-library" / "2.0.6-abcdef012345"
    shutil.copytree(w.qap, snap / "library")
    r = _run(_argv(c), {"XDG_CACHE_HOME": str(tmp_path / "xdg")}, home=tmp_path / "home")
    assert r.returncode == 0 and r.stdout.strip().endswith("\ntrue"), (r.stdout, r.stderr)
    rt = tmp_path / "runtime"
    (rt / "bin").mkdir(parents=True)
    shutil.copy(VERIFY, rt / "bin" / "verify")                                    # alone: it needs no library next to it
    shutil.copytree(w.qap, rt / "resource" / "qap-compiler" / "library")
    env = {k: v for k, v in os.environ.items() if k not in ("TKMK_SUBCIRCUIT_LIBRARY", "XDG_CACHE_HOME")}
    env["HOME"] = str(tmp_path / "home")
    r = subprocess.run([str(rt / "bin" / "verify")] + _argv(c), capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("\ntrue"), (r.stdout, r.stderr)
    # usage errors
    r = _run(["--crs", "a", "--synthesizer-stat", "b", "--proof", "d"])
    assert r.returncode == 2 and "--preprocess <PATH>" in r.stderr and "Usage: verify" in r.stderr
    r = _run(_argv(c) + ["--output", "x"])
    assert r.returncode == 2 and "unexpected argument '--output'" in r.stderr
    r = _run(_argv(c) + ["--crs", "again"])
    assert r.returncode == 2 and "cannot be used multiple times" in r.stderr
    r = _run(["--crs", "a", "--synthesizer-stat", "b", "--preprocess", "c", "--proof"])
    assert r.returncode == 2 and "a value is required" in r.stderr
    r = _run(_argv(c) + ["--subcircuit-library", str(tmp_path / "nowhere")])
    assert r.returncode == 1 and "cannot resolve subcircuit library path" in r.stderr
    r = _run(["--help"])
    assert r.returncode == 0 and r.stdout.startswith("Usage: verify")
    for flag in ("--version", "-V"):
        r = _run([flag])
        assert r.returncode == 0 and r.stdout.startswith("verify ")
        assert re.search(r"\b\d+\.\d+\.\d+(?:[-+][0-9A-Za-z.-]+)?\b", r.stdout).group(0).startswith("2.1.3")
