"""CPU tier: batch verification on the host route — tkmk_verify_batch_files (include/tkmk_prover.h, tkmk.verify.verify_batch) and
`bin/verify --batch`, both over verify_batch of host/tkmk_verify.hpp — on the files of two distinct honest proofs of one small circuit made
by the restated prover of tests/prove_ref.py with two mixers (the shape of tests/test_verify_native.py: s_max = 8, m_I > 2); further
items are copies or tampered variants.

What is asserted is structural: an all-honest batch costs ONE pairing product; a verdict is per proof and equals what tkmk_verify_files
says for that item alone, with the same reason; b false items among N cost at most 1 + 2 b ceil(log2 N) products; two tampered proofs
whose errors would cancel under equal weights are both found; membership is never folded; an unreadable document and an empty batch are
errors, not verdicts."""
import copy
import json
import os
import random
import subprocess

import numpy as np
import pytest

from test_verify_native import G2_NAMES, PINS, VERIFY, World, _case, _run

R_EVAL_KEYS = ("thetas", "kappa0", "chi", "zeta", "kappa1", "a_eval")


@pytest.fixture(scope="module")
def world(oracle, tkmk, tmp_path_factory):
    import prove_ref
    import synth_circuit
    from tkmk import g2, proofio
    from tkmk.prove import random_mixer
    w = World()
    w.tmp = tmp_path_factory.mktemp("verify_batch")
    w.R = oracle.R_MOD
    g = oracle.to_bytes([int(PINS["fixed_tau_g1_x"], 16), int(PINS["fixed_tau_g1_y"], 16)], 48)
    h = g2.from_hex_pair(PINS["fixed_tau_g2_x"], PINS["fixed_tau_g2_y"])
    inst = synth_circuit.build(str(w.tmp), random.Random(17), s_max=8, n_gate_kinds=2, used_placements=7)
    w.sp, w.qap, w.synth, w.instance = inst["setup_params"], inst["qap"], inst["synth"], inst["instance"]
    assert w.sp["l_D"] - w.sp["l"] > 2
    w.tau = {k: int(PINS["tau_" + k], 16) for k in ("x", "y", "alpha", "gamma", "delta", "eta")}
    crs = prove_ref.sigma_gen(inst, w.tau)
    w.rec = lambda dlog: np.asarray(prove_ref.g1_of(dlog, g))                          # noqa: E731
    w.crs_g1 = {"G": w.rec(1), "x": w.rec(crs["tau_x"]), "y": w.rec(crs["tau_y"]), "lagrange_KL": w.rec(crs["lagrange_KL"])}
    w.sigma2 = dict(zip(G2_NAMES, g2.sigma2_gen(w.tau, h)))
    w.proofio, w.g2, w.h = proofio, g2, h
    w.proofs = []
    for seed in (17, 18):                                                               # two mixers: two distinct honest proofs
        d, s, ch, p4t, rp = prove_ref.run(inst, crs, random_mixer(random.Random(seed)), g)
        w.proofs.append({"dlog": d, "points": {k: w.rec(v) for k, v in d.items()}, "scalars": dict(s)})
        if seed == 17:
            w.pre_points = {k: w.rec(v) for k, v in prove_ref.preprocess(rp, inst, crs).items()}
    assert any((w.proofs[0]["points"][k] != w.proofs[1]["points"][k]).any() for k in w.proofs[0]["points"])
    w.dlog, w.points, w.scalars = w.proofs[0]["dlog"], w.proofs[0]["points"], w.proofs[0]["scalars"]      # what _case takes as "honest"
    w.honest = [_case(w, "honest0"), _case(w, "honest1", points=w.proofs[1]["points"], scalars=w.proofs[1]["scalars"])]
    w.negated = _case(w, "negated", points=dict(w.points, Pi_X=np.asarray(oracle.g1_neg(w.points["Pi_X"].copy()))))
    return w


def _item(c):
    return (c["synth"], c["pre"], c["proof"])


def _batch(w, cases, **kw):
    from tkmk import verify
    each, rep = verify.verify_batch(w.qap, cases[0]["crs"], [_item(c) for c in cases], **kw)
    assert rep["n"] == len(cases) == len(rep["items"]) == len(each) and rep["route"] == "host"
    assert rep["ok"] == all(each) and [it["ok"] for it in rep["items"]] == each
    assert set(rep["seconds"]) == {"parse", "membership", "fold", "pairings", "total"}
    return each, rep


def _single(w, c):
    from tkmk import verify
    return verify.verify_files(w.qap, c["crs"], c["synth"], c["pre"], c["proof"])


def _agrees_with_single(w, cases, each, rep):
    """every verdict and reason equals tkmk_verify_files on that item alone; the challenges too where the single report has them"""
    for k, c in enumerate(cases):
        ok, one = _single(w, c)
        it = rep["items"][k]
        assert each[k] == ok and it["reason"] == one["reason"] and set(it) == set(one), (k, it, one)
        for key in R_EVAL_KEYS:
            assert it.get(key) == one.get(key), (k, key)


@pytest.mark.parametrize("n", [1, 2, 5])
def test_all_honest_is_one_product(world, n):
    w = world
    cases = [w.honest[k % 2] for k in range(n)]
    each, rep = _batch(w, cases)
    assert each == [True] * n and rep["products"] == 1 and rep["ok"] is True
    _agrees_with_single(w, cases, each, rep)
    assert all(it["reason"] == "" and "thetas" in it for it in rep["items"])
    if n >= 2:
        assert rep["items"][0]["chi"] != rep["items"][1]["chi"]                        # two distinct proofs


@pytest.mark.parametrize("pos", range(5))
def test_one_false_item_at_each_position(world, pos):
    w = world
    cases = [w.honest[k % 2] for k in range(5)]
    cases[pos] = w.negated
    each, rep = _batch(w, cases)
    assert each == [k != pos for k in range(5)]
    assert 2 <= rep["products"] <= 1 + 2 * 3                                         # 1 + 2 b ceil(log2 5), b = 1
    assert rep["items"][pos]["reason"] == "pairing product != 1"
    if pos == 0:
        _agrees_with_single(w, cases, each, rep)


def test_cancelling_pair_is_found(world):
    """O_mid is not in the transcript and enters the equation through e(-O_mid, eta) alone: [d + 1]G in one copy and [d - 1]G in the other
    are errors of +G and -G that cancel in a fold with EQUAL weights.  With independent weights both are false."""
    w = world
    d = w.dlog["O_mid"]
    plus = _case(w, "o_mid_plus", points=dict(w.points, O_mid=w.rec((d + 1) % w.R)))
    minus = _case(w, "o_mid_minus", points=dict(w.points, O_mid=w.rec((d - 1) % w.R)))
    cases = [plus, minus, w.honest[1]]
    for _ in range(2):                                                                  # fresh weights every call
        each, rep = _batch(w, cases)
        assert each == [False, False, True], rep
        assert rep["products"] <= 1 + 2 * 2 * 2
    _agrees_with_single(w, cases, each, rep)


def test_membership_is_per_item_and_never_folded(world, oracle):
    import g1_torsion
    w, P = world, oracle.P_MOD
    stray = g1_torsion.torsion_point(11, random.Random(3))                              # on the curve, order 11
    assert g1_torsion.on_curve(stray) and not g1_torsion.in_subgroup(stray)
    cofactor = _case(w, "b_cofactor", points=dict(w.points, Q_CX=g1_torsion.to_record(*stray)))
    # a small-order component ADDED to an honest point: the pairing does not see it, only the membership check does
    x, y = oracle.to_ints(w.proofs[1]["points"]["O_prv"], 48)
    mixed = g1_torsion.add((int(x), int(y)), g1_torsion.torsion_point(3, random.Random(4)))
    hidden = _case(w, "b_hidden", points=dict(w.proofs[1]["points"], O_prv=g1_torsion.to_record(*mixed)), scalars=w.proofs[1]["scalars"])
    doc = w.proofio.format_proof(w.points, w.scalars)
    qx, _ = oracle.to_ints(w.points["Q_AY"], 48)
    be = int(qx + P).to_bytes(48, "big")
    i = 2 * w.proofio.PROOF_POINT_ORDER.index("Q_AY")
    doc["proof_entries_part1"][i], doc["proof_entries_part2"][i] = "0x" + be[:16].hex(), "0x" + be[16:].hex()
    not_reduced = _case(w, "b_not_reduced", proof_doc=doc)
    cases = [w.honest[0], cofactor, w.honest[1], not_reduced, hidden]
    each, rep = _batch(w, cases)
    assert each == [True, False, True, False, False] and rep["products"] == 1           # the bad items enter no fold
    assert rep["items"][1]["reason"] == "proof.json: Q_CX is not in the subgroup of order r"
    assert rep["items"][3]["reason"] == "proof.json: Q_AY has a coordinate that is not reduced (>= p)"
    assert rep["items"][4]["reason"] == "proof.json: O_prv is not in the subgroup of order r"
    _agrees_with_single(w, cases, each, rep)
    # a bad record of the shared preprocess: every item that names it is false, the item with its own preprocess is not
    off = dict(w.pre_points, s1=g1_torsion.to_record(*stray))
    bad_pre = _case(w, "b_pre", pre_points=off)
    cases = [bad_pre, w.honest[0], dict(w.honest[1], pre=bad_pre["pre"])]
    each, rep = _batch(w, cases)
    assert each == [False, True, False] and rep["products"] == 1
    assert rep["items"][0]["reason"] == rep["items"][2]["reason"] == "preprocess.json: s1 is not in the subgroup of order r"
    _agrees_with_single(w, cases, each, rep)


def test_wrong_instance_flipped_evaluation_and_all_false(world):
    w = world
    ins = copy.deepcopy(w.instance)
    ins["a_pub_user"][0] = hex((int(ins["a_pub_user"][0], 16) + 1) % w.R)
    wrong_instance = _case(w, "b_instance", instance=ins)
    flipped = _case(w, "b_r_eval", scalars=dict(w.scalars, R_eval=(w.scalars["R_eval"] + 1) % w.R))
    each, rep = _batch(w, [w.honest[1], wrong_instance, w.honest[0]])
    assert each == [True, False, True] and rep["products"] <= 1 + 2 * 2
    assert rep["items"][1]["a_eval"] != rep["items"][2]["a_eval"] and rep["items"][1]["chi"] == rep["items"][2]["chi"]
    each, rep = _batch(w, [w.honest[0], w.honest[1], flipped])
    assert each == [True, True, False] and rep["products"] <= 1 + 2 * 2
    cases = [w.negated, wrong_instance, flipped, w.negated]
    each, rep = _batch(w, cases)
    assert each == [False] * 4 and rep["ok"] is False and rep["products"] <= 1 + 2 * 4 * 2
    _agrees_with_single(w, cases, each, rep)


def test_sigma2_refuses_the_whole_batch(world):
    w = world
    c = _case(w, "b_no_sigma2", sigma2={k: None for k in G2_NAMES})
    cases = [dict(w.honest[0], crs=c["crs"]), dict(w.honest[1], crs=c["crs"])]
    each, rep = _batch(w, cases)
    assert each == [False, False] and rep["products"] == 0
    assert all("holds no Sigma2" in it["reason"] and "thetas" not in it for it in rep["items"])
    c = _case(w, "b_no_alpha", sigma2=dict(w.sigma2, alpha=None))
    each, rep = _batch(w, [dict(w.honest[0], crs=c["crs"])])
    assert each == [False] and "sigma_2.alpha is the point at infinity" in rep["items"][0]["reason"]


def test_unreadable_document_and_empty_batch_are_errors(world):
    from tkmk import service, verify
    w = world
    broken = _case(w, "b_unreadable")
    open(os.path.join(broken["proof"], "proof.json"), "w").write('{"proof_entries_part1": [')
    with pytest.raises(service.ProverError) as e:
        _batch(w, [w.honest[0], w.honest[1], broken, w.honest[0]])
    assert e.value.code == 11 and "item 2" in str(e.value) and "proof.json" in str(e.value), str(e.value)
    os.remove(os.path.join(broken["proof"], "proof.json"))
    with pytest.raises(service.ProverError) as e:
        _batch(w, [w.honest[0], w.honest[1], broken])
    assert "item 2" in str(e.value) and "No proof is found. Run the Prove first." in str(e.value) and "proof.json" in str(e.value)
    with pytest.raises(service.ProverError) as e:
        verify.verify_batch(w.qap, w.honest[0]["crs"], [])
    assert e.value.code == 11                                                           # TKMK_ERR_INVALID_ARGUMENT: no vacuous "all true"


def test_device_route_without_a_device_is_refused(world, tkmk):
    from tkmk import service, verify
    if tkmk.device_count() > 0:
        pytest.skip("a GPU is visible")
    w = world
    with pytest.raises(service.ProverError) as e:
        verify.verify_batch(w.qap, w.honest[0]["crs"], [_item(w.honest[0])], route="device")
    assert e.value.code == 12                                                           # TKMK_ERR_NO_DEVICE


def test_binary_batch_mode(world, tmp_path):
    w = world
    cases = [w.honest[0], w.negated, w.honest[1]]
    manifest = tmp_path / "manifest.json"
    json.dump([{"synthesizer-stat": c["synth"], "preprocess": c["pre"], "proof": c["proof"]} for c in cases], open(manifest, "w"))
    env = {"TKMK_SUBCIRCUIT_LIBRARY": w.qap}
    r = _run(["--batch", str(manifest), "--crs", w.honest[0]["crs"]], env)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.strip().split("\n")
    assert lines[-6:-4] == ["Verifier initialization...", "Verifying the proof..."], r.stdout
    assert lines[-4:] == ["0 true", "1 false", "2 true", "false"], r.stdout
    assert "item 1: pairing product != 1" in r.stderr and "root-of-unity generator" in r.stderr
    each, rep = _batch(w, cases)
    assert ["%d %s" % (k, "true" if v else "false") for k, v in enumerate(each)] == lines[-4:-1]
    json.dump([{"synthesizer-stat": c["synth"], "preprocess": c["pre"], "proof": c["proof"]} for c in w.honest], open(manifest, "w"))
    r = _run(["--batch=" + str(manifest), "--crs", w.honest[0]["crs"], "--subcircuit-library", w.qap])
    assert r.returncode == 0 and r.stdout.strip().split("\n")[-3:] == ["0 true", "1 true", "true"], (r.stdout, r.stderr)
    # usage errors: exit status 2
    for extra in (["--proof", cases[0]["proof"]], ["--preprocess", cases[0]["pre"]], ["--synthesizer-stat", cases[0]["synth"]]):
        r = _run(["--batch", str(manifest), "--crs", w.honest[0]["crs"]] + extra, env)
        assert r.returncode == 2 and "--batch" in r.stderr and "Usage: verify" in r.stderr, r.stderr
    # input errors: exit status 1, no verdict line
    open(manifest, "w").write("[]")
    r = _run(["--batch", str(manifest), "--crs", w.honest[0]["crs"]], env)
    assert r.returncode == 1 and r.stdout.strip().split("\n")[-1] not in ("true", "false"), (r.stdout, r.stderr)
    r = _run(["--batch", str(tmp_path / "nowhere.json"), "--crs", w.honest[0]["crs"]], env)
    assert r.returncode == 1 and "nowhere.json" in r.stderr
    r = subprocess.run(["ldd", VERIFY], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "libtkmk_hip" not in r.stdout and "libamdhip64" not in r.stdout and "libhsa" not in r.stdout, r.stdout
