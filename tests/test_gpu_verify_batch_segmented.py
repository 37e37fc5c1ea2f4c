"""gpu tier: the device route of batch verification with its small slot jobs on the segmented small-MSM entry
(host/tkmk_verify_device.hpp: the jobs of at most kSegmentedMaxTerms terms in one tkmk_msm_segmented call, the rest in one
tkmk_msm_multi_ex call).  The fixture is the recipe of tests/test_gpu_verify_batch.py — the s_max = 8 synthetic circuit, one resident
context, a handful of its proofs — rebuilt here.  Verdicts, reasons and the number of pairing products equal the host route's, and the
report's two job counters account for every slot job of every fold."""
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
SLOTS = 10                                                                              # slot jobs per fold (tkmk::verify::kSlots)


class World:
    pass


@pytest.fixture(scope="module")
def world(gpu, oracle, tmp_path_factory):
    import synth_circuit
    from tkmk import proofio, service
    w = World()
    w.tmp = tmp_path_factory.mktemp("gpu_verify_batch_segmented")
    w.inst = synth_circuit.build(str(w.tmp), random.Random(73), s_max=8, n_gate_kinds=2, used_placements=7, bit_fraction=0.4)
    w.crs_dir, w.pre = str(w.tmp / "crs"), str(w.tmp / "pre")
    os.makedirs(w.crs_dir), os.makedirs(w.pre)
    env = {k: v for k, v in os.environ.items() if k not in ("TKMK_FR_ROOT_GENERATOR", "TKMK_SUBCIRCUIT_LIBRARY")}
    for cmd in ([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", w.inst["qap"], "--output", w.crs_dir],
                [os.path.join(BIN, "preprocess"), "--crs", w.crs_dir, "--synthesizer-stat", w.inst["synth"], "--output", w.pre, "--subcircuit-library", w.inst["qap"]]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (cmd, r.stderr)
    w.synth = w.inst["synth"]
    w.ctx = service.Prover(w.inst["qap"], w.crs_dir, testing=True)
    w.honest = []
    for k in range(4):                                                                  # four proofs, four draws of the blinding scalars
        out = w.tmp / ("proof%d" % k)
        out.mkdir()
        w.ctx.prove(w.synth, str(out), want_json=False)
        w.honest.append(str(out))
    points, scalars = proofio.recover_proof(json.load(open(os.path.join(w.honest[0], "proof.json"))))
    w.negated = str(w.tmp / "negated")
    os.makedirs(w.negated)
    proofio.write_json(os.path.join(w.negated, "proof.json"),
                       proofio.format_proof(dict(points, Pi_X=np.asarray(oracle.g1_neg(points["Pi_X"].copy()))), scalars))
    yield w
    w.ctx.close()


def _both_routes(w, proofs):
    from tkmk import verify
    items = [(w.synth, w.pre, p) for p in proofs]
    host, hrep = verify.verify_batch_with(w.ctx, items, route="host")
    dev, drep = verify.verify_batch_with(w.ctx, items, route="device")
    assert hrep["route"] == "host" and drep["route"] == "device"
    assert dev == host and drep["ok"] == hrep["ok"] == all(dev)
    assert drep["products"] == hrep["products"]
    assert [it["reason"] for it in drep["items"]] == [it["reason"] for it in hrep["items"]]
    assert hrep["segmented_jobs"] == 0 and hrep["pipeline_jobs"] == 0                   # the host route calls neither entry
    # every fold of these batches has terms (each holds an item that passed membership), and every fold is one pairing product
    assert drep["segmented_jobs"] > 0
    assert drep["segmented_jobs"] + drep["pipeline_jobs"] == SLOTS * drep["products"]
    return dev, drep


def test_one_item(world):
    each, rep = _both_routes(world, world.honest[:1])
    assert each == [True] and rep["products"] == 1
    assert rep["segmented_jobs"] + rep["pipeline_jobs"] == SLOTS


def test_three_items_one_false(world):
    w = world
    each, rep = _both_routes(w, [w.honest[0], w.negated, w.honest[1]])
    assert each == [True, False, True] and 2 <= rep["products"] <= 1 + 2 * 2
    assert rep["items"][1]["reason"] == "pairing product != 1"


def test_eight_items_all_honest(world):
    w = world
    each, rep = _both_routes(w, [w.honest[k % 4] for k in range(8)])
    assert each == [True] * 8 and rep["products"] == 1
    assert rep["segmented_jobs"] >= 6                                                   # six of the ten slot jobs have one term at every batch size
