"""gpu tier: the witness check on a sharded prover (tkmk_prover_check_witness_sharded, TKMK_PROVER_CHECK_WITNESS=1 inside a sharded
tkmk_prover_prove; host/tkmk_witness_check.hpp run_sharded) with G = 2, 4, 8 virtual ranks over the loopback transport.

The world is that of tests/test_gpu_witness_check.py — the same synth_circuit.generate(...) shape, the same mutations, the Python-integer
checker `expected` imported from that module — under another seed, because the sharded copy section needs more of its inputs than the
single-GPU one does: a failing entry whose value crosses ranks, a rank that owns no failing entry, an entry that stays on its rank
(test_the_documents_exercise_the_exchange, plain Python over the documents).  SEED = 515 is the first seed from 1 up for which that holds
for every G, in each of the two copy cases and in their union; it was searched for with the checker alone, before any device ran.

The single-GPU report of tkmk_prover_check_witness is the reference: the existing tests tie it to the checker and to the verifier.  Here
every rank's report must equal it key for key outside "seconds".  `many_faults` is new: every placement's variables shifted by
placement + 1, which breaks all 8 placements (the shape has 8: no more can be bad), 17 of the 20 copy entries with destinations on every
column — so on every rank of every G — and all 8 public wires: the merge has more than 8 copy findings to order and cut, and 8
arithmetic findings that arrive from all ranks.  That case is held against `expected` once more.

The communicator keeps no count of its exchanges (tkmk_comm_describe reports transport, size, rank and device only), so the number of
collectives a check adds is not asserted here."""
import copy
import json
import os
import random
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "tokamak-zk-evm_amd", "bin")
KNOB = "TKMK_PROVER_CHECK_WITNESS"
SEED = 515
WORLDS = [2, 4, 8]
CASES = ["honest", "arithmetic", "arithmetic_p7", "copy", "copy_values", "not_bijection", "public_user", "public_function", "two_faults", "many_faults"]


class World:
    pass


def _documents():
    """the circuit and the ten document sets, from Python alone -> (inst, {name: (pv, perm, instance)})"""
    import synth_circuit
    from test_gpu_witness_check import R, _plus_one, expected
    inst = synth_circuit.generate(random.Random(SEED), s_max=8, n_gate_kinds=2, used_placements=8, bit_fraction=0.0)
    pv, perm, instance = inst["placement_variables"], inst["permutation"], inst["instance"]
    b, subs = expected(inst, pv, perm, instance)["b"], inst["subs"]
    docs = {}

    def case(name, pv=pv, perm=perm, instance=instance):
        docs[name] = (pv, perm, instance)

    def bumped(q, wire):
        out = copy.deepcopy(pv)
        out[q]["variables"][wire] = _plus_one(out[q]["variables"][wire])
        return out
    # the mutations of tests/test_gpu_witness_check.py's fixture, one by one
    case("honest")
    case("arithmetic", pv=bumped(4, -1))
    case("arithmetic_p7", pv=bumped(7, -1))
    i, j = next((i, j) for i in range(len(perm)) for j in range(i + 1, len(perm)) if b[perm[i]["X"]][perm[i]["Y"]] != b[perm[j]["X"]][perm[j]["Y"]])
    swapped = copy.deepcopy(perm)
    for k in ("X", "Y"):
        swapped[i][k], swapped[j][k] = perm[j][k], perm[i][k]
    case("copy", perm=swapped)
    sub4 = subs[pv[4]["subcircuitId"]]
    first_in = list(sub4.ins())[0]
    old = [int(h, 16) for h in pv[4]["variables"]]
    moved = copy.deepcopy(pv)
    moved[4]["variables"] = ["0x%x" % v for v in sub4.witness([old[wire] + (1 if wire == first_in else 0) for wire in sub4.ins()])]
    case("copy_values", pv=moved)
    folded = copy.deepcopy(perm)
    folded[0]["X"], folded[0]["Y"] = perm[1]["X"], perm[1]["Y"]
    case("not_bijection", perm=folded)
    pub_user = copy.deepcopy(instance)
    pub_user["a_pub_user"][0] = _plus_one(pub_user["a_pub_user"][0])
    case("public_user", instance=pub_user)
    pub_fn = copy.deepcopy(instance)
    pub_fn["a_pub_function"][0] = _plus_one(pub_fn["a_pub_function"][0])
    case("public_function", instance=pub_fn)
    case("two_faults", pv=bumped(4, -1), instance=pub_user)
    shifted = copy.deepcopy(pv)                                                # every variable of placement q moved by q + 1
    for q, p in enumerate(shifted):
        p["variables"] = ["0x%x" % ((int(v, 16) + q + 1) % R) for v in p["variables"]]
    case("many_faults", pv=shifted)
    assert sorted(docs) == sorted(CASES)
    return inst, docs


@pytest.fixture(scope="module")
def documents():
    return _documents()


def test_the_documents_exercise_the_exchange(documents):
    """from the documents alone: for every G, in `copy`, in `copy_values` and in the two together, a failing entry's value crosses ranks
    (col mod G != Y mod G) and some rank owns no failing entry; some entry of the permutation stays on its rank; and `many_faults` gives
    every rank of every G bad placements and failing entries, more than 8 of the latter"""
    from test_gpu_witness_check import expected
    inst, docs = documents
    sp = inst["setup_params"]
    assert min(sp["n"], sp["l_D"] - sp["l"], sp["s_max"]) >= max(WORLDS)         # no G is skipped at this shape
    failing = {}
    for name in ("copy", "copy_values", "many_faults"):
        pv, perm, instance = docs[name]
        want = expected(inst, pv, perm, instance)
        assert want["entries"] and want["bijection"]
        assert want["n_entries"] == len(perm)                                    # no duplicate destination: entry k is perm[k]
        failing[name] = [(perm[e]["col"], perm[e]["Y"]) for e in want["entries"]]
    failing["both"] = failing["copy"] + failing["copy_values"]
    perm = docs["honest"][1]
    for G in WORLDS:
        for name in ("copy", "copy_values", "both"):
            assert any(col % G != y % G for col, y in failing[name]), (G, name)
            assert len({col % G for col, _ in failing[name]}) < G, (G, name)
        assert any(e["col"] % G == e["Y"] % G for e in perm), G
        assert {col % G for col, _ in failing["many_faults"]} == set(range(G))
    pv, perm, instance = docs["many_faults"]
    want = expected(inst, pv, perm, instance)
    assert sorted(want["rows"]) == list(range(8)) and len(want["entries"]) > 8 and len(want["public"]) == 8


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("TKMK_FR_ROOT_GENERATOR", "TKMK_HOST_TRACE", "TKMK_PROVER_CHECK_CRS", KNOB, "TKMK_SUBCIRCUIT_LIBRARY")}


def _without_seconds(rep):
    return {k: v for k, v in rep.items() if k != "seconds"}


@pytest.fixture(scope="module")
def world(gpu, documents, tmp_path_factory):
    """one circuit, one `trusted-setup --fixed-tau`, one single-GPU context of the testing library; the sharded contexts are opened once
    per G, on first use (world.ranks(G)), and live to the end of the module"""
    import synth_circuit
    from test_gpu_prove import seeded_mixer
    from test_gpu_service import _mixer_file
    from test_gpu_witness_check import expected
    from tkmk import dist, service, verify
    w = World()
    w.tmp = tmp_path_factory.mktemp("witness_check_sharded")
    w.inst, docs = documents
    synth_circuit.write(w.inst, str(w.tmp), synth_files=False)
    w.qap = w.inst["qap"]
    w.crs = str(w.tmp / "crs")
    os.makedirs(w.crs)
    r = subprocess.run([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", w.qap, "--output", w.crs], capture_output=True, text=True, timeout=600,
                       env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr
    w.mixer = _mixer_file(w.tmp, seeded_mixer(SEED))
    w.cases = {}
    for name, (pv, perm, instance) in docs.items():
        d = w.tmp / name / "synth"
        os.makedirs(d)
        for doc, body in (("placementVariables.json", pv), ("permutation.json", perm), ("instance.json", instance)):
            json.dump(body, open(d / doc, "w"))
        w.cases[name] = dict(synth=str(d), want=expected(w.inst, pv, perm, instance))
    os.environ.pop(KNOB, None)
    w.single = service.Prover(w.qap, w.crs, testing=True)
    w.single_proof, _ = w.single.prove(w.cases["honest"]["synth"], None, testing_mixer_json=w.mixer)
    reports, opened = {}, {}

    def single_report(name):                                                   # tkmk_prover_check_witness on the single-GPU context, once per case
        if name not in reports:
            reports[name] = verify.witness_check(None, w.cases[name]["synth"], prover=w.single)
        return reports[name]

    def ranks(G):
        if G not in opened:
            comms = dist.loopback_comms(G)
            opened[G] = (comms, None)                                          # closed below even when an open fails
            provers = dist.run_ranks(comms, lambda c: service.Prover(w.qap, w.crs, testing=True, comm=c))
            opened[G] = (comms, {p.comm.rank: p for p in provers})
        return opened[G]
    w.single_report, w.ranks = single_report, ranks
    yield w
    for comms, by_rank in opened.values():
        for p in (by_rank or {}).values():
            p.close()
        for c in comms:
            c.close()
    w.single.close()


def _collective_check(world, G, synth):
    from tkmk import dist, verify
    comms, by_rank = world.ranks(G)
    return dist.run_ranks(comms, lambda c: verify.witness_check(None, synth, prover=by_rank[c.rank], collective=True))


@pytest.mark.parametrize("G", WORLDS)
@pytest.mark.parametrize("name", CASES)
def test_every_ranks_report_equals_the_single_gpu_report(world, name, G):
    ok, rep = world.single_report(name)
    want = world.cases[name]["want"]
    clean = not want["rows"] and not want["entries"] and want["bijection"] and not want["public"]
    assert ok == rep["ok"] == clean                                             # the reference itself against the checker's verdict
    res = _collective_check(world, G, world.cases[name]["synth"])
    assert len(res) == G
    for rank, (ok_r, rep_r) in enumerate(res):
        assert ok_r == ok, (rank, rep_r["reason"])
        assert set(rep_r) == set(rep) and set(rep_r["seconds"]) == set(rep["seconds"])
        for key in rep:
            if key != "seconds":
                assert rep_r[key] == rep[key], (rank, key)


def test_many_faults_single_gpu_report_against_the_checker(world):
    from test_gpu_witness_check import _agrees_with_checker
    ok, rep = world.single_report("many_faults")
    want = world.cases["many_faults"]["want"]
    _agrees_with_checker(rep, want, world.inst)
    assert not ok and rep["reason"].startswith("arithmetic: placement 0 ")
    assert len(rep["arithmetic"]["first"]) == 8 and len(rep["copy"]["first"]) == 8 and rep["copy"]["bad_entries"] == len(want["entries"]) > 8
    assert [f["entry"] for f in rep["copy"]["first"]] == want["entries"][:8]
    assert len(rep["public"]["first"]) == 8


def test_world_of_one_is_the_unsharded_entry(world):
    """the collective entry on a context from tkmk_prover_open, and on the one rank of a one-rank communicator"""
    from tkmk import dist, service, verify
    for name in ("honest", "two_faults", "copy_values"):
        ok, rep = world.single_report(name)
        ok1, rep1 = verify.witness_check(None, world.cases[name]["synth"], prover=world.single, collective=True)
        assert ok1 == ok and _without_seconds(rep1) == _without_seconds(rep)
    comms = dist.loopback_comms(1)
    try:
        with service.Prover(world.qap, world.crs, testing=True, comm=comms[0]) as alone:
            for name in ("honest", "many_faults"):
                ok, rep = world.single_report(name)
                ok1, rep1 = verify.witness_check(None, world.cases[name]["synth"], prover=alone, collective=True)
                assert ok1 == ok and _without_seconds(rep1) == _without_seconds(rep)
    finally:
        comms[0].close()


def _prove_all(world, G, synth, out_of_rank0=None):
    from tkmk import dist
    comms, by_rank = world.ranks(G)
    return dist.run_ranks(comms, lambda c: by_rank[c.rank].prove(synth, out_of_rank0 if c.rank == 0 else None, testing_mixer_json=world.mixer)[0])


@pytest.mark.parametrize("G", [2, 4])
def test_knob_refuses_on_every_rank_and_changes_no_byte_of_an_honest_proof(world, monkeypatch, G):
    from tkmk import dist, service
    comms, by_rank = world.ranks(G)
    honest = world.cases["honest"]["synth"]
    monkeypatch.delenv(KNOB, raising=False)
    unset = _prove_all(world, G, honest)
    assert all(d == world.single_proof for d in unset)
    monkeypatch.setenv(KNOB, "1")
    for name in ("arithmetic", "copy_values", "public_function"):
        out = str(world.tmp / ("refused_%s_%d" % (name, G)))

        def attempt(c):
            try:
                by_rank[c.rank].prove(world.cases[name]["synth"], out if c.rank == 0 else None, testing_mixer_json=world.mixer)
            except service.ProverError as e:
                return e.code, str(e)
            return None
        res = dist.run_ranks(comms, attempt)
        reason = world.single_report(name)[1]["reason"]
        assert reason
        assert all(r is not None for r in res), (name, res)
        assert [r[0] for r in res] == [11] * G, (name, res)
        assert len({r[1] for r in res}) == 1 and reason in res[0][1] and KNOB in res[0][1], (name, res)
        assert not os.path.exists(os.path.join(out, "proof.json"))
    out = str(world.tmp / ("knob_out_%d" % G))
    docs = _prove_all(world, G, honest, out_of_rank0=out)                      # the same contexts, the knob still set
    for d in docs:
        assert d == unset[0] and d == world.single_proof
    assert json.load(open(os.path.join(out, "proof.json"))) == docs[0]


@pytest.mark.parametrize("G", [2, 4])
def test_a_check_between_two_proofs_changes_no_byte_of_the_second(world, monkeypatch, G):
    monkeypatch.delenv(KNOB, raising=False)
    res = _collective_check(world, G, world.cases["arithmetic"]["synth"])
    assert [ok for ok, _ in res] == [False] * G
    assert all(d == world.single_proof for d in _prove_all(world, G, world.cases["honest"]["synth"]))


@pytest.mark.parametrize("G", [2, 4])
def test_an_unreadable_permutation_is_every_ranks_error_naming_the_file(world, monkeypatch, G):
    from tkmk import dist, service, verify
    monkeypatch.delenv(KNOB, raising=False)
    comms, by_rank = world.ranks(G)
    d = str(world.tmp / ("no_permutation_%d" % G))
    shutil.copytree(world.cases["honest"]["synth"], d)
    os.remove(os.path.join(d, "permutation.json"))

    def attempt(c):
        try:
            verify.witness_check(None, d, prover=by_rank[c.rank], collective=True)
        except service.ProverError as e:
            return str(e)
        return None
    res = dist.run_ranks(comms, attempt)
    assert all(r is not None and "permutation.json" in r for r in res), res
    assert all(doc == world.single_proof for doc in _prove_all(world, G, world.cases["honest"]["synth"]))
    res = _collective_check(world, G, world.cases["honest"]["synth"])          # and they check afterwards
    assert [ok for ok, _ in res] == [True] * G


@pytest.mark.parametrize("G", [2, 4])
def test_an_input_error_only_the_owner_of_a_placement_sees_is_every_ranks_error(world, monkeypatch, G):
    """instance.json without a_pub_function: the public wires that map into it belong to one of placements 0..3, whose values only
    rank (placement mod G) staged — that rank alone can find the value missing.  The text travels in its block of the merge: every rank
    raises it, it is the single-GPU context's text, and the contexts check and prove afterwards (the communicator was not aborted)"""
    from tkmk import dist, service, verify
    monkeypatch.delenv(KNOB, raising=False)
    comms, by_rank = world.ranks(G)
    d = str(world.tmp / ("no_function_values_%d" % G))
    shutil.copytree(world.cases["honest"]["synth"], d)
    instance = json.load(open(os.path.join(d, "instance.json")))
    assert instance["a_pub_function"]
    instance["a_pub_function"] = []
    json.dump(instance, open(os.path.join(d, "instance.json"), "w"))
    with pytest.raises(service.ProverError) as single:
        verify.witness_check(None, d, prover=world.single)
    assert single.value.code == 11 and "instance.json: no value for public wire" in str(single.value)
    text = str(single.value).split("failed: ", 1)[1]

    def attempt(c):
        try:
            verify.witness_check(None, d, prover=by_rank[c.rank], collective=True)
        except service.ProverError as e:
            return e.code, str(e).split("failed: ", 1)[1]
        return None
    assert dist.run_ranks(comms, attempt) == [(11, text)] * G
    res = _collective_check(world, G, world.cases["honest"]["synth"])
    assert [ok for ok, _ in res] == [True] * G
    assert all(doc == world.single_proof for doc in _prove_all(world, G, world.cases["honest"]["synth"]))


def test_the_uncollective_entry_still_refuses_and_names_the_collective_one(world):
    from tkmk import service, verify
    _, by_rank = world.ranks(2)
    for p in by_rank.values():                                                  # rank after rank: the entry is not collective
        with pytest.raises(service.ProverError) as e:
            verify.witness_check(None, world.cases["honest"]["synth"], prover=p)
        assert e.value.code == 11 and "sharded" in str(e.value) and "tkmk_prover_check_witness_sharded" in str(e.value)
