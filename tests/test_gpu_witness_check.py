"""gpu tier: the witness check (host/tkmk_witness_check.hpp: tkmk_witness_check_files, tkmk_prover_check_witness, bin/witness-check,
TKMK_PROVER_CHECK_WITNESS=1 inside tkmk_prover_prove).  One small circuit, one `trusted-setup --fixed-tau` and one resident context of
the testing library with a fixed mixer, as tests/test_gpu_crs_audit.py builds its world.  Every case is a copy of the three per-proof
documents with one fault (or none); a checker in this file recomputes the complete expected findings from the documents with Python
integers, and the VERIFIER is the ground truth: for every case `ok` must equal tkmk_prover_verify's verdict on the proof the unguarded
prover makes from the same documents (bin/preprocess runs on the case's documents too).  The unguarded prover of those comparisons is a
second context, of the PRODUCTION library: the testing-mode build measures every polynomial's degree against its bound
(host/tkmk_host.hpp shape_degree) and so refuses most bad witnesses by itself, with "degree bound violated", before there is a proof to
verify; the production build makes the proof the issue is about.  A verdict does not depend on the blinding scalars."""
import copy
import json
import os
import random
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "tokamak-zk-evm_amd", "bin")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
KNOB = "TKMK_PROVER_CHECK_WITNESS"


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("TKMK_FR_ROOT_GENERATOR", "TKMK_HOST_TRACE", "TKMK_PROVER_CHECK_CRS", KNOB, "TKMK_SUBCIRCUIT_LIBRARY")}
    env.update({k: str(v) for k, v in extra.items()})
    return env


def _run(cmd, **extra):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=_env(**extra), cwd=ROOT)


# ------------------------------------------------------------------------------------------------ the checker: Python integers only
def expected(inst, pv, perm, instance):
    """-> dict(rows = {placement: [failing rows]}, entries = [failing indices of the effective permutation], bijection, public =
    [failing public indices], n_entries, n_public) from the documents alone"""
    sp, subs = inst["setup_params"], inst["subs"]
    l, s_max, m_i = sp["l"], sp["s_max"], sp["l_D"] - sp["l"]
    vals = [[int(h, 16) for h in p["variables"]] for p in pv]
    dot = lambda lc, w: sum(c * w[k] for k, c in lc) % R                                         # noqa: E731
    rows = {}
    for q, p in enumerate(pv):
        bad = [i for i, (A, B, C) in enumerate(subs[p["subcircuitId"]].rows) if dot(A, vals[q]) * dot(B, vals[q]) % R != dot(C, vals[q])]
        if bad:
            rows[q] = bad
    b = [[0] * s_max for _ in range(m_i)]
    for q, p in enumerate(pv):
        for wire, g in enumerate(subs[p["subcircuitId"]].flatten_map):
            if l <= g < l + m_i:
                b[g - l][q] = vals[q][wire]
    last = {}
    for e in perm:                                                                              # the last writer of a cell wins
        last[(e["row"], e["col"])] = (e["X"], e["Y"])
    seen, effective = set(), []
    for e in reversed(perm):
        cell = (e["row"], e["col"])
        if cell not in seen:
            seen.add(cell)
            effective.append((cell, last[cell]))
    if len(effective) == len(perm):
        effective = [((e["row"], e["col"]), (e["X"], e["Y"])) for e in perm]                    # no duplicate: file order
    image = [src for _, src in effective] + [(r, c) for r in range(m_i) for c in range(s_max) if (r, c) not in seen]
    entries = [k for k, ((r, c), (x, y)) in enumerate(effective) if b[r][c] != b[x][y]]
    a_pub = [int(h, 16) for h in instance["a_pub_user"][:sp["l_user"]] + instance["a_pub_block"][:sp["l_free"] - sp["l_user"]] + instance["a_pub_function"]]
    public, n_public = [], 0
    for q in range(4):
        s = subs[pv[q]["subcircuitId"]]
        for wire in (s.outs() if s.name == "bufferPubOut" else s.ins()):
            n_public += 1
            if vals[q][wire] != a_pub[s.flatten_map[wire]]:
                public.append(s.flatten_map[wire])
    return dict(rows=rows, entries=entries, bijection=len(set(image)) == len(image), public=sorted(public), n_entries=len(effective), n_public=n_public, b=b)


class World:
    pass


def _plus_one(h):
    return "0x%x" % ((int(h, 16) + 1) % R)


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    import synth_circuit
    from test_gpu_prove import seeded_mixer
    from test_gpu_service import _mixer_file
    from tkmk import service
    w = World()
    w.tmp = tmp_path_factory.mktemp("witness_check")
    inst = synth_circuit.generate(random.Random(83), s_max=8, n_gate_kinds=2, used_placements=8, bit_fraction=0.0)
    synth_circuit.write(inst, str(w.tmp), synth_files=False)
    w.inst, w.qap = inst, inst["qap"]
    w.crs = str(w.tmp / "crs")
    os.makedirs(w.crs)
    r = _run([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", w.qap, "--output", w.crs])
    assert r.returncode == 0, r.stderr
    w.mixer = _mixer_file(w.tmp, seeded_mixer(83))
    pv, perm, instance = inst["placement_variables"], inst["permutation"], inst["instance"]
    honest = expected(inst, pv, perm, instance)
    assert honest["rows"] == {} and honest["entries"] == [] and honest["bijection"] and honest["public"] == [] and honest["n_entries"] == 21
    b, subs = honest["b"], inst["subs"]
    w.cases = {}

    def case(name, pv=pv, perm=perm, instance=instance):
        d = w.tmp / name
        os.makedirs(d / "synth")
        for doc, body in (("placementVariables.json", pv), ("permutation.json", perm), ("instance.json", instance)):
            json.dump(body, open(d / "synth" / doc, "w"))
        w.cases[name] = dict(synth=str(d / "synth"), pre=str(d / "pre"), out=str(d / "out"), want=expected(inst, pv, perm, instance), docs=(pv, perm, instance))

    def bumped(q, wire):
        out = copy.deepcopy(pv)
        out[q]["variables"][wire] = _plus_one(out[q]["variables"][wire])
        return out
    case("honest")
    case("arithmetic", pv=bumped(4, -1))                                       # the last private wire of placement 4
    case("arithmetic_p7", pv=bumped(7, -1))
    first_in = list(subs[pv[4]["subcircuitId"]].ins())[0]
    case("arithmetic_input", pv=bumped(4, first_in))
    i, j = next((i, j) for i in range(len(perm)) for j in range(i + 1, len(perm)) if b[perm[i]["X"]][perm[i]["Y"]] != b[perm[j]["X"]][perm[j]["Y"]])
    swapped = copy.deepcopy(perm)
    for k in ("X", "Y"):
        swapped[i][k], swapped[j][k] = perm[j][k], perm[i][k]
    case("copy", perm=swapped)
    sub4 = subs[pv[4]["subcircuitId"]]
    old = [int(h, 16) for h in pv[4]["variables"]]
    forward = sub4.witness([old[wire] + (1 if wire == first_in else 0) for wire in sub4.ins()])
    moved = copy.deepcopy(pv)
    moved[4]["variables"] = ["0x%x" % v for v in forward]
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
    # the mutations listed for this seed
    assert w.cases["arithmetic"]["want"]["rows"] == {4: [5, 6, 7]}
    assert w.cases["arithmetic_p7"]["want"]["rows"] == {7: [5, 6]}
    assert w.cases["arithmetic_input"]["want"]["rows"] == {4: [0, 1, 2, 3, 7]}
    w.ctx = service.Prover(w.qap, w.crs, testing=True)
    w.plain = service.Prover(w.qap, w.crs)                                      # the production library: the unguarded prover of the ground truth
    os.environ.pop(KNOB, None)
    w.honest_doc, _ = w.ctx.prove(w.cases["honest"]["synth"], None, testing_mixer_json=w.mixer)
    yield w
    w.plain.close()
    w.ctx.close()


def _check_all_entries(world, name):
    """the verdict and report of the case through both library entries; they must agree"""
    from tkmk import verify
    c = world.cases[name]
    ok, rep = verify.witness_check(world.qap, c["synth"], testing=True)
    ok2, rep2 = verify.witness_check(None, c["synth"], prover=world.ctx)
    assert ok == ok2 == rep["ok"] == rep2["ok"]
    for sec in ("arithmetic", "copy", "public"):
        assert rep[sec] == rep2[sec]
    assert rep["reason"] == rep2["reason"]
    assert set(rep["seconds"]) == {"parse", "upload", "build", "check", "total"}
    return ok, rep


def _agrees_with_checker(rep, want, inst):
    a, c, p = rep["arithmetic"], rep["copy"], rep["public"]
    assert a["placements"] == 8 and a["bad_placements"] == len(want["rows"]) and a["bad_cells"] == sum(len(v) for v in want["rows"].values())
    assert [(f["placement"], f["first_row"], f["bad_rows"]) for f in a["first"]] == [(q, rows[0], len(rows)) for q, rows in sorted(want["rows"].items())]
    assert a["ok"] == (not want["rows"])
    for f in a["first"]:
        info = inst["infos"][inst["placement_variables"][f["placement"]]["subcircuitId"]]
        assert (f["subcircuitId"], f["name"]) == (info["id"], info["name"])
        u, v, w_ = (int(f[k], 16) for k in "uvw")
        assert all(len(f[k]) == 66 for k in "uvw") and u * v % R != w_
    assert c["entries"] == want["n_entries"] and c["bijection"] == want["bijection"] and c["bad_entries"] == len(want["entries"])
    assert [f["entry"] for f in c["first"]] == want["entries"][:8]
    assert c["ok"] == (want["bijection"] and not want["entries"])
    for f in c["first"]:
        assert want["b"][f["row"]][f["col"]] == int(f["value"], 16) != int(f["source"], 16) == want["b"][f["X"]][f["Y"]]
    assert p["wires"] == want["n_public"] and p["bad"] == len(want["public"]) and sorted(f["index"] for f in p["first"]) == want["public"][:8]
    assert p["ok"] == (not want["public"])


# (arithmetic_p7 and arithmetic_input exist for the checker's own pins in the fixture; the eight below go to the device and the verifier)
CASES = ["honest", "arithmetic", "copy", "copy_values", "not_bijection", "public_user", "public_function", "two_faults"]
TARGET = {"arithmetic": "rows", "arithmetic_p7": "rows", "arithmetic_input": "rows", "copy": "entries", "copy_values": "entries", "public_user": "public",
          "public_function": "public"}


@pytest.mark.parametrize("name", CASES)
def test_report_equals_the_checker_and_ok_equals_the_verifier(world, name):
    """the findings against the checker of this file, and the GROUND TRUTH: bin/preprocess on the case's documents, one proof with the
    knob unset, tkmk_prover_verify's verdict = the check's ok"""
    from tkmk import verify
    c = world.cases[name]
    want = c["want"]
    if name in TARGET:
        assert want[TARGET[name]], "the mutation must break the section it targets"
    if name == "not_bijection":
        assert not want["bijection"]
    if name == "two_faults":
        assert want["rows"] and want["public"]
    ok, rep = _check_all_entries(world, name)
    print(name, "check:", ok, rep["reason"])
    _agrees_with_checker(rep, want, world.inst)
    clean = not want["rows"] and not want["entries"] and want["bijection"] and not want["public"]
    assert ok == clean and (rep["reason"] == "") == clean
    os.makedirs(c["pre"])
    r = _run([os.path.join(BIN, "preprocess"), "--crs", world.crs, "--synthesizer-stat", c["synth"], "--output", c["pre"], "--subcircuit-library", world.qap])
    assert r.returncode == 0, r.stderr
    assert KNOB not in os.environ
    world.plain.prove(c["synth"], c["out"], want_json=False)
    assert os.path.exists(os.path.join(c["out"], "proof.json"))
    verdict, vrep = verify.prover_verify(world.plain, c["synth"], c["pre"], c["out"])
    print(name, "verifier:", verdict, vrep.get("reason"))
    assert verdict == ok, (name, rep["reason"], vrep.get("reason"))


def test_honest_witness_through_the_binary_without_a_crs(world):
    c = world.cases["honest"]
    argv = [os.path.join(BIN, "witness-check"), "--synthesizer-stat", c["synth"], "--subcircuit-library", world.qap]
    assert "--crs" not in argv and world.crs not in argv
    r = _run(argv)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "true" and [ln.split(":")[0] for ln in lines[-4:-1]] == ["arithmetic", "copy", "public"]
    assert all(" ok " in ln for ln in lines[-4:-1])


def test_sections_are_named_by_the_binary(world):
    r = _run([os.path.join(BIN, "witness-check"), "--synthesizer-stat", world.cases["two_faults"]["synth"], "--subcircuit-library", world.qap])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "false" and "FAILED" in lines[-4] and " ok " in lines[-3] and "FAILED" in lines[-2]
    assert "arithmetic: placement 4" in r.stderr and "public: index 0" in r.stderr


def test_single_section_cases_leave_the_other_sections_clean(world):
    for name, dirty in (("arithmetic", "arithmetic"), ("copy", "copy"), ("copy_values", "copy"), ("not_bijection", "copy"), ("public_user", "public")):
        want = world.cases[name]["want"]
        flags = {"arithmetic": not want["rows"], "copy": want["bijection"] and not want["entries"], "public": not want["public"]}
        assert [s for s, ok in flags.items() if not ok] == [dirty], name
    _, rep = _check_all_entries(world, "copy")
    assert rep["copy"]["bijection"] is True and rep["arithmetic"]["ok"] and rep["public"]["ok"]
    _, rep = _check_all_entries(world, "not_bijection")
    assert rep["copy"]["bijection"] is False and "hit_twice" in rep["copy"] and "not a bijection" in rep["reason"]
    _, rep = _check_all_entries(world, "two_faults")
    assert not rep["arithmetic"]["ok"] and not rep["public"]["ok"] and rep["copy"]["ok"] and rep["reason"].startswith("arithmetic: placement 4 ")


def test_knob_refuses_a_bad_witness_and_changes_no_byte_of_an_honest_proof(world, monkeypatch):
    from tkmk import service
    honest, bad = world.cases["honest"], world.cases["arithmetic"]
    monkeypatch.setenv(KNOB, "1")
    doc, _ = world.ctx.prove(honest["synth"], None, testing_mixer_json=world.mixer)
    assert doc == world.honest_doc
    out = str(world.tmp / "refused_out")
    with pytest.raises(service.ProverError) as e:
        world.ctx.prove(bad["synth"], out, testing_mixer_json=world.mixer)
    info = world.inst["infos"][world.inst["placement_variables"][4]["subcircuitId"]]
    assert e.value.code == 11 and "placement 4 " in str(e.value) and info["name"] in str(e.value) and "row 5" in str(e.value)
    assert not os.path.exists(os.path.join(out, "proof.json"))
    doc, _ = world.ctx.prove(honest["synth"], None, testing_mixer_json=world.mixer)          # the context stays usable
    assert doc == world.honest_doc
    out = str(world.tmp / "refused_out_production")
    with pytest.raises(service.ProverError) as e:                                            # the production library reads the knob too
        world.plain.prove(bad["synth"], out)
    assert e.value.code == 11 and "placement 4 " in str(e.value) and info["name"] in str(e.value)
    assert not os.path.exists(os.path.join(out, "proof.json"))
    monkeypatch.setenv(KNOB, "0")
    world.plain.prove(bad["synth"], out, want_json=False)                                    # 0 is unset: the unguarded prover
    assert os.path.exists(os.path.join(out, "proof.json"))


def test_a_check_between_two_proofs_changes_no_byte_of_the_second(world):
    from tkmk import verify
    ok, _ = verify.witness_check(None, world.cases["arithmetic"]["synth"], prover=world.ctx)
    assert ok is False
    doc, _ = world.ctx.prove(world.cases["honest"]["synth"], None, testing_mixer_json=world.mixer)
    assert doc == world.honest_doc


def test_unreadable_input_is_an_error_naming_the_file(world):
    import shutil
    from tkmk import service, verify
    d = str(world.tmp / "no_permutation")
    shutil.copytree(world.cases["honest"]["synth"], d)
    os.remove(os.path.join(d, "permutation.json"))
    for kw in (dict(testing=True), dict(prover=world.ctx)):
        with pytest.raises(service.ProverError) as e:
            verify.witness_check(world.qap, d, **kw)
        assert "permutation.json" in str(e.value)
    r = _run([os.path.join(BIN, "witness-check"), "--synthesizer-stat", d, "--subcircuit-library", world.qap])
    assert r.returncode == 1 and "permutation.json" in r.stderr and r.stdout.strip().splitlines()[-1] not in ("true", "false")
    r = _run([os.path.join(BIN, "witness-check"), "--subcircuit-library", world.qap])
    assert r.returncode == 2 and "Usage: witness-check" in r.stderr


def test_a_sharded_context_refuses(world):
    from tkmk import dist, service, verify
    comms = dist.loopback_comms(2)
    provers = dist.run_ranks(comms, lambda c: service.Prover(world.qap, world.crs, testing=True, comm=c))
    try:
        for p in provers:
            with pytest.raises(service.ProverError) as e:
                verify.witness_check(None, world.cases["honest"]["synth"], prover=p)
            assert e.value.code == 11 and "sharded" in str(e.value)
    finally:
        for p in provers:
            p.close()
        for c in comms:
            c.close()


def test_real_library_honest_pass(gpu, tmp_path):
    import real_library
    from tkmk import verify
    lib = real_library.assemble(str(tmp_path / "library"))
    made = real_library.make_inputs(str(tmp_path / "synth"), random.Random(2031))
    ok, rep = verify.witness_check(lib, str(tmp_path / "synth"))
    assert ok, rep["reason"]
    assert rep["arithmetic"]["placements"] == len(made["order"])
