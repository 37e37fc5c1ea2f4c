"""gpu tier: batch verification through the device route (host/tkmk_verify_device.hpp: upload of the distinct records, one tkmk_g1_check,
one tkmk_msm_multi_ex per fold, the pairing on the host) on one resident context of the s_max = 8 synthetic circuit and five proofs it
made.  Every verdict, every reason and the number of pairing products equal the host route's on the same items; a batch that is no power
of two carries identical bases under different scalars inside one MSM job; the context proves the same bytes before and after; a sharded
context keeps the host route and refuses the device route.  In-process, like the other tests of this tier."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "tokamak-zk-evm_amd", "bin")


class World:
    pass


@pytest.fixture(scope="module")
def world(gpu, oracle, tmp_path_factory):
    import synth_circuit
    from tkmk import proofio, service
    w = World()
    w.tmp = tmp_path_factory.mktemp("gpu_verify_batch")
    w.inst = synth_circuit.build(str(w.tmp), random.Random(73), s_max=8, n_gate_kinds=2, used_placements=7, bit_fraction=0.4)
    assert w.inst["setup_params"]["l_D"] - w.inst["setup_params"]["l"] > 2
    w.crs_dir, w.pre = str(w.tmp / "crs"), str(w.tmp / "pre")
    os.makedirs(w.crs_dir), os.makedirs(w.pre)
    env = {k: v for k, v in os.environ.items() if k not in ("TKMK_FR_ROOT_GENERATOR", "TKMK_SUBCIRCUIT_LIBRARY")}
    for cmd in ([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", w.inst["qap"], "--output", w.crs_dir],      # writes sigma_verify.json too
                [os.path.join(BIN, "preprocess"), "--crs", w.crs_dir, "--synthesizer-stat", w.inst["synth"], "--output", w.pre, "--subcircuit-library", w.inst["qap"]]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (cmd, r.stderr)
    w.synth, w.proofio = w.inst["synth"], proofio
    w.ctx = service.Prover(w.inst["qap"], w.crs_dir, testing=True)
    w.honest = []
    for k in range(5):                                                                  # five proofs, five draws of the blinding scalars
        out = w.tmp / ("proof%d" % k)
        out.mkdir()
        w.ctx.prove(w.synth, str(out), want_json=False)
        w.honest.append(str(out))
    w.points, w.scalars = proofio.recover_proof(json.load(open(os.path.join(w.honest[0], "proof.json"))))
    assert len({open(os.path.join(d, "proof.json")).read() for d in w.honest}) == 5
    w.oracle = oracle
    yield w
    w.ctx.close()


def _variant(w, name, points=None, scalars=None, doc=None):
    d = w.tmp / name
    if not d.exists():
        d.mkdir()
        w.proofio.write_json(d / "proof.json", doc or w.proofio.format_proof(points or w.points, scalars or w.scalars))
    return str(d)


def _negated(w):
    return _variant(w, "negated", points=dict(w.points, Pi_X=np.asarray(w.oracle.g1_neg(w.points["Pi_X"].copy()))))


def _both_routes(w, proofs):
    """the same items through both routes of tkmk_prover_verify_batch -> (verdicts, the device route's report)"""
    from tkmk import verify
    items = [(w.synth, w.pre, p) for p in proofs]
    host, hrep = verify.verify_batch_with(w.ctx, items, route="host")
    dev, drep = verify.verify_batch_with(w.ctx, items, route="device")
    assert hrep["route"] == "host" and drep["route"] == "device" and drep["n"] == hrep["n"] == len(proofs)
    assert dev == host and drep["ok"] == hrep["ok"] == all(dev)
    assert drep["products"] == hrep["products"]
    assert drep["generator"] == hrep["generator"] == w.ctx.root_generator
    for a, b in zip(drep["items"], hrep["items"]):
        assert a["ok"] == b["ok"] and a["reason"] == b["reason"] and set(a) == set(b), (a, b)
        for key in ("thetas", "kappa0", "chi", "zeta", "kappa1", "a_eval"):
            assert a.get(key) == b.get(key)
    return dev, drep


@pytest.mark.parametrize("n", [1, 5])
def test_all_honest_is_one_product_on_the_device(world, n):
    from tkmk import verify
    w = world
    each, rep = _both_routes(w, w.honest[:n])
    assert each == [True] * n and rep["products"] == 1
    ok, one = verify.prover_verify(w.ctx, w.synth, w.pre, w.honest[0])                  # the single verifier on item 0
    assert ok and {k: one[k] for k in ("thetas", "chi", "zeta", "kappa1", "a_eval")} == {k: rep["items"][0][k] for k in ("thetas", "chi", "zeta", "kappa1", "a_eval")}


@pytest.mark.parametrize("pos", [0, 4])
def test_one_false_item_first_and_last(world, pos):
    w = world
    proofs = list(w.honest)
    proofs[pos] = _negated(w)
    each, rep = _both_routes(w, proofs)
    assert each == [k != pos for k in range(5)] and 2 <= rep["products"] <= 1 + 2 * 3
    assert rep["items"][pos]["reason"] == "pairing product != 1"


def test_cancelling_pair_and_all_false(world):
    """O_mid + T in one copy, O_mid - T in the other, T a fixed point of the subgroup: under equal weights the two errors cancel"""
    w, o = world, world.oracle
    t = w.points["U"]
    plus = _variant(w, "o_mid_plus", points=dict(w.points, O_mid=np.asarray(o.g1_add(w.points["O_mid"].copy(), t.copy()))))
    minus = _variant(w, "o_mid_minus", points=dict(w.points, O_mid=np.asarray(o.g1_add(w.points["O_mid"].copy(), np.asarray(o.g1_neg(t.copy()))))))
    each, rep = _both_routes(w, [plus, minus, w.honest[1]])
    assert each == [False, False, True] and rep["products"] <= 1 + 2 * 2 * 2
    flipped = _variant(w, "r_eval", scalars=dict(w.scalars, R_eval=(w.scalars["R_eval"] + 1) % o.R_MOD))
    each, rep = _both_routes(w, [_negated(w), plus, flipped, minus])
    assert each == [False] * 4 and rep["products"] <= 1 + 2 * 4 * 2


def test_membership_failures_have_the_single_verifiers_reasons(world):
    import g1_torsion
    from tkmk import verify
    w, o = world, world.oracle
    stray = g1_torsion.torsion_point(11, random.Random(3))
    cofactor = _variant(w, "cofactor", points=dict(w.points, Q_CX=g1_torsion.to_record(*stray)))
    x, y = o.to_ints(w.points["O_prv"], 48)
    mixed = g1_torsion.add((int(x), int(y)), g1_torsion.torsion_point(3, random.Random(4)))
    hidden = _variant(w, "hidden", points=dict(w.points, O_prv=g1_torsion.to_record(*mixed)))        # the pairing would not see this
    off = _variant(w, "off_curve", points=dict(w.points, W=g1_torsion.to_record(int(x), (int(y) + 1) % o.P_MOD)))
    doc = w.proofio.format_proof(w.points, w.scalars)
    qx, _ = o.to_ints(w.points["Q_AY"], 48)
    be = int(qx + o.P_MOD).to_bytes(48, "big")
    i = 2 * w.proofio.PROOF_POINT_ORDER.index("Q_AY")
    doc["proof_entries_part1"][i], doc["proof_entries_part2"][i] = "0x" + be[:16].hex(), "0x" + be[16:].hex()
    not_reduced = _variant(w, "not_reduced", doc=doc)
    proofs = [w.honest[1], cofactor, not_reduced, w.honest[2], hidden, off]
    each, rep = _both_routes(w, proofs)
    assert each == [True, False, False, True, False, False] and rep["products"] == 1
    assert rep["items"][1]["reason"] == "proof.json: Q_CX is not in the subgroup of order r"
    assert rep["items"][2]["reason"] == "proof.json: Q_AY has a coordinate that is not reduced (>= p)"
    assert rep["items"][4]["reason"] == "proof.json: O_prv is not in the subgroup of order r"
    assert rep["items"][5]["reason"] == "proof.json: W is not on the curve"
    for k in (1, 2):
        ok, one = verify.prover_verify(w.ctx, w.synth, w.pre, proofs[k])
        assert not ok and one["reason"] == rep["items"][k]["reason"] and "thetas" not in rep["items"][k]


def test_33_items_two_false(world):
    """not a power of two; 31 copies of five proofs: identical bases under different scalars inside one MSM job"""
    from tkmk import verify
    w = world
    proofs = [w.honest[k % 5] for k in range(33)]
    flipped = _variant(w, "r_eval", scalars=dict(w.scalars, R_eval=(w.scalars["R_eval"] + 1) % w.oracle.R_MOD))
    proofs[7], proofs[32] = _negated(w), flipped
    each, rep = verify.verify_batch_with(w.ctx, [(w.synth, w.pre, p) for p in proofs], route="device")
    assert each == [k not in (7, 32) for k in range(33)] and rep["route"] == "device" and rep["n"] == 33
    assert 3 <= rep["products"] <= 1 + 2 * 2 * 6
    print("33 items, 2 false, device route:", rep["products"], "products,", rep["seconds"])


def test_the_context_is_untouched(world, tkmk):
    """the same fixed-mixer proof before and after a device-route batch, byte for byte; the NTT domain and the generator in effect too"""
    from test_gpu_prove import seeded_mixer
    from tkmk import verify
    w = world
    hx = lambda v: [hx(e) for e in v] if isinstance(v, list) else "0x%x" % v          # noqa: E731
    mixer_path = str(w.tmp / "mixer.json")
    json.dump({k: hx(v) for k, v in seeded_mixer(29).items()}, open(mixer_path, "w"))
    before, _ = w.ctx.prove(w.synth, None, testing_mixer_json=mixer_path)
    state = (tkmk.root_generator(), w.ctx.root_generator)
    each, rep = verify.verify_batch_with(w.ctx, [(w.synth, w.pre, p) for p in w.honest[:3] + [_negated(w)]], route="device")
    assert each == [True, True, True, False]
    after, _ = w.ctx.prove(w.synth, None, testing_mixer_json=mixer_path)
    assert json.dumps(after, sort_keys=True) == json.dumps(before, sort_keys=True)
    assert (tkmk.root_generator(), w.ctx.root_generator) == state
    out = w.tmp / "after"
    out.mkdir()
    w.ctx.prove(w.synth, str(out), testing_mixer_json=mixer_path, want_json=False)
    assert verify.verify_batch_with(w.ctx, [(w.synth, w.pre, str(out))], route="device")[0] == [True]


def test_files_entry_on_the_device_route(world):
    """tkmk_verify_batch_files with TKMK_VERIFY_ROUTE_DEVICE: sigma_verify.json instead of a context's reference string"""
    from tkmk import verify
    w = world
    items = [(w.synth, w.pre, p) for p in (w.honest[0], _negated(w), w.honest[3])]
    each, rep = verify.verify_batch(w.inst["qap"], w.crs_dir, items, root_generator=w.ctx.root_generator, route="device")
    assert each == [True, False, True] and rep["route"] == "device" and rep["products"] <= 1 + 2 * 2
    host, hrep = verify.verify_batch(w.inst["qap"], w.crs_dir, items, root_generator=w.ctx.root_generator, route="host")
    assert host == each and hrep["products"] == rep["products"] and [it["reason"] for it in hrep["items"]] == [it["reason"] for it in rep["items"]]


def test_sharded_context_keeps_the_host_route(world):
    from tkmk import dist, service, verify
    w = world
    comms = dist.loopback_comms(2)
    provers = dist.run_ranks(comms, lambda c: service.Prover(w.inst["qap"], w.crs_dir, testing=True, comm=c))
    by_rank = {p.comm.rank: p for p in provers}
    try:
        items = [(w.synth, w.pre, p) for p in w.honest[:3]]
        for rank in (0, 1):                                                             # no collective: a rank verifies alone
            each, rep = verify.verify_batch_with(by_rank[rank], items, route="host")
            assert each == [True] * 3 and rep["products"] == 1 and rep["route"] == "host"
        with pytest.raises(service.ProverError) as e:
            verify.verify_batch_with(by_rank[0], items, route="device")
        assert e.value.code == 11 and "sharded" in str(e.value)
    finally:
        for p in provers:
            p.close()
        for c in comms:
            c.close()
