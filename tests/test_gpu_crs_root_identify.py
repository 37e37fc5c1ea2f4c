"""gpu tier: the root-of-unity convention of a CRS is IDENTIFIED at open, then adopted or refused (include/tkmk.h tkmk_crs_identify_root;
host/tkmk_prover.hpp identify_crs_root; include/tkmk_prover.h tkmk_prover_open).

lagrange_KL = [L_{s_max-1}(tau_y) K_{m_I-1}(tau_x)] G follows from xy_powers under exactly one of the two candidate generators
(5: ffjavascript's rule, declared; 7: arkworks / zkcrypto), so a CRS says which one it was made under.  The small circuit of
tests/test_root_convention.py; `trusted-setup --fixed-tau` and `preprocess` run once under TKMK_FR_ROOT_GENERATOR=7 (and the setup once
more without it), everything below then runs WITHOUT the variable — removed from the child's environment, not left to luck — on the
g = 7 CRS.  Whatever switches the process-wide generator runs in a child process: the pytest process keeps the declared one."""
import json
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BIN = os.path.join(ROOT, "tokamak-zk-evm_amd", "bin")


def _env(gen=None):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tokamak-zk-evm_amd"), HERE, os.path.join(ROOT, "tools")]))
    env.pop("TKMK_FR_ROOT_GENERATOR", None)
    env.pop("TKMK_HOST_TRACE", None)
    if gen is not None:
        env["TKMK_FR_ROOT_GENERATOR"] = str(gen)
    return env


def _run(cmd, gen=None):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=_env(gen), cwd=ROOT)


def _py(code, args, gen=None):
    r = _run([sys.executable, "-c", code] + [str(a) for a in args], gen)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


class World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """circuit + CRS made under g = 7 (whole directory, archive only, flat payload only) + CRS made under the default + a CRS whose
    lagrange_KL record is replaced by G + the preprocess made under the override: built once, read-only afterwards"""
    import synth_circuit
    from tkmk import crs as crsmod
    w = World()
    tmp = tmp_path_factory.mktemp("crs_root")
    w.tmp = str(tmp)
    inst = synth_circuit.build(w.tmp, random.Random(81), s_max=8, n_gate_kinds=2, used_placements=8, bit_fraction=0.4)
    w.qap, w.synth = inst["qap"], inst["synth"]
    w.sp = inst["setup_params"]
    for name in ("crs7", "crs5", "crs7_rkyv", "crs7_tkcrs", "corrupt", "pre7"):
        os.makedirs(os.path.join(w.tmp, name))
        setattr(w, name, os.path.join(w.tmp, name))
    for crs, gen in ((w.crs7, 7), (w.crs5, None)):
        r = _run([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", w.qap, "--output", crs], gen)
        assert r.returncode == 0, r.stderr
    shutil.copy(os.path.join(w.crs7, "combined_sigma.rkyv"), w.crs7_rkyv)
    shutil.copy(os.path.join(w.crs7, "combined_sigma.tkcrs"), w.crs7_tkcrs)
    r = _run([os.path.join(BIN, "preprocess"), "--crs", w.crs7, "--synthesizer-stat", w.synth, "--output", w.pre7, "--subcircuit-library", w.qap], 7)
    assert r.returncode == 0, r.stderr
    w.preprocess7 = open(os.path.join(w.pre7, "preprocess.json"), "rb").read()
    sec = dict(crsmod.read_payload(os.path.join(w.crs5, "combined_sigma.tkcrs")))
    g1 = bytearray(bytes(sec["g1"]))
    g1[5 * 96:6 * 96] = g1[0:96]                                           # lagrange_KL := G
    sec["g1"] = bytes(g1)
    open(os.path.join(w.corrupt, "combined_sigma.tkcrs"), "wb").write(crsmod.build_payload(sec))
    return w


def _out(world, name):
    d = os.path.join(world.tmp, name)
    os.makedirs(d, exist_ok=True)
    return d


def _args(world, crs, out):
    return ["--crs", crs, "--synthesizer-stat", world.synth, "--output", out, "--subcircuit-library", world.qap]


# ---------------------------------------------------------------------------------------------------------------------------------
# the entry: sums per candidate, no comparison, no state
# ---------------------------------------------------------------------------------------------------------------------------------
def _affine(gpu, proj):
    return gpu.projective_to_affine_bytes(proj).reshape(-1, 96)


@pytest.mark.parametrize("made_under", [7, 5])
def test_entry_tells_the_generator_a_crs_was_made_under(gpu, oracle, world, made_under):
    from tkmk import crs as crsmod
    sec = crsmod.read_payload(os.path.join(world.crs7 if made_under == 7 else world.crs5, "combined_sigma.tkcrs"))
    sp = world.sp
    m_i, s_max = sp["l_D"] - sp["l"], sp["s_max"]
    h_max, rs_y = max(2 * sp["n"], 2 * m_i), 2 * s_max
    kl = np.asarray(crsmod.single_g1(sec, "lagrange_KL"))
    xy = gpu.DeviceBuffer.from_host(np.ascontiguousarray(sec["xy_powers"]))
    before = gpu.root_generator()
    whole = _affine(gpu, gpu.crs_identify_root(xy, h_max, rs_y, m_i, s_max, (5, 7)))
    other = 5 if made_under == 7 else 7
    by_gen = {5: whole[0], 7: whole[1]}
    assert (by_gen[made_under] == kl).all() and not (by_gen[other] == kl).all()
    # a sharded rank's share: columns 0, 2, 4, ... and 1, 3, 5, ...; the partials add up to the whole sum
    even = _affine(gpu, gpu.crs_identify_root(xy, h_max, rs_y, m_i, s_max, (5, 7), col0=0, col_step=2))
    odd = _affine(gpu, gpu.crs_identify_root(xy, h_max, rs_y, m_i, s_max, (5, 7), col0=1, col_step=2))
    for c in range(2):
        assert not (even[c] == whole[c]).all()
        assert (oracle.g1_add(even[c].copy(), odd[c].copy()) == whole[c]).all(), c
    # the same on the table in the MSM's resident form (what a context holds after its conversion pass), in the other candidate order
    conv = gpu.msm_convert_bases(xy)
    again = _affine(gpu, gpu.crs_identify_root(conv, h_max, rs_y, m_i, s_max, (7, 5), bases_form=gpu.BASES_CONVERTED))
    assert (again[0] == by_gen[7]).all() and (again[1] == by_gen[5]).all()
    assert gpu.root_generator() == before                                  # the entry changes no state
    # arguments: a residue among the candidates, a corner larger than the table, no candidate
    for kw, cand in ((dict(), (5, 4)), (dict(), ()), (dict(col_step=0), (5,))):
        with pytest.raises(gpu.TkmkError) as e:
            gpu.crs_identify_root(xy, h_max, rs_y, m_i, s_max, cand, **kw)
        assert e.value.code == 11
    with pytest.raises(gpu.TkmkError) as e:
        gpu.crs_identify_root(xy, h_max, rs_y, 2 * h_max, s_max, (5, 7))
    assert e.value.code == 11


# ---------------------------------------------------------------------------------------------------------------------------------
# the binaries
# ---------------------------------------------------------------------------------------------------------------------------------
VERIFY_CODE = """
import json, sys
import verify_files
print(json.dumps(bool(verify_files.verify(*sys.argv[1:5]))))
"""


@pytest.mark.parametrize("container", ["rkyv", "tkcrs"])
def test_prove_adopts_the_generator_of_the_crs(world, container):
    crs = world.crs7_rkyv if container == "rkyv" else world.crs7_tkcrs
    assert os.listdir(crs) == ["combined_sigma." + container]
    out = _out(world, "out_prove_" + container)
    r = _run([os.path.join(BIN, "prove")] + _args(world, crs, out))
    assert r.returncode == 0, r.stderr
    assert "generator 7" in r.stderr, r.stderr
    open(os.path.join(out, "preprocess.json"), "wb").write(world.preprocess7)
    assert _py(VERIFY_CODE, [world.qap, world.synth, world.crs7, out], gen=7) is True


def test_preprocess_adopts_the_generator_of_the_crs(world):
    for crs, name in ((world.crs7, "whole"), (world.crs7_tkcrs, "tkcrs")):
        out = _out(world, "out_pre_" + name)
        r = _run([os.path.join(BIN, "preprocess")] + _args(world, crs, out))
        assert r.returncode == 0, r.stderr
        assert "generator 7" in r.stderr
        assert open(os.path.join(out, "preprocess.json"), "rb").read() == world.preprocess7, name
    # the archives alone (sigma_preprocess.rkyv is what `preprocess` reads; combined_sigma.rkyv next to it carries lagrange_KL)
    both = _out(world, "crs7_archives")
    for f in ("combined_sigma.rkyv", "sigma_preprocess.rkyv"):
        shutil.copy(os.path.join(world.crs7, f), both)
    out = _out(world, "out_pre_archives")
    r = _run([os.path.join(BIN, "preprocess")] + _args(world, both, out))
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(out, "preprocess.json"), "rb").read() == world.preprocess7


def test_corrupted_crs_is_refused_by_the_prover_and_a_warning_for_preprocess(gpu, world):
    from tkmk import service
    with pytest.raises(service.ProverError) as e:
        service.Prover(world.qap, world.corrupt)
    assert e.value.code == 11 and "5" in str(e.value) and "7" in str(e.value) and "lagrange_KL" in str(e.value), str(e.value)
    assert gpu.root_generator() == 5                                       # nothing was switched
    out = _out(world, "out_corrupt")
    r = _run([os.path.join(BIN, "prove")] + _args(world, world.corrupt, out))
    assert r.returncode != 0 and "lagrange_KL" in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(out, "proof.json"))
    r = _run([os.path.join(BIN, "preprocess")] + _args(world, world.corrupt, out))
    assert r.returncode == 0 and "warning" in r.stderr and "lagrange_KL" in r.stderr, r.stderr
    want = _out(world, "out_pre5")                                         # ... and went on under the generator in effect
    assert _run([os.path.join(BIN, "preprocess")] + _args(world, world.crs5, want)).returncode == 0
    assert open(os.path.join(out, "preprocess.json"), "rb").read() == open(os.path.join(want, "preprocess.json"), "rb").read()


def test_a_pinned_generator_is_not_overridden(world):
    out = _out(world, "out_pinned")
    r = _run([os.path.join(BIN, "prove")] + _args(world, world.crs7, out), gen=5)
    assert r.returncode != 0 and "TKMK_FR_ROOT_GENERATOR" in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(out, "proof.json"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the library (testing build, fixed blinding scalars), each scenario in a child process of its own
# ---------------------------------------------------------------------------------------------------------------------------------
LIB_CODE = """
import json, os, random, sys
import tkmk
from tkmk import dist, service
from tkmk.prove import random_mixer
mode, qap, synth, tmp, crs = sys.argv[1:6]
tkmk.set_device(0)
hx = lambda v: [hx(e) for e in v] if isinstance(v, list) else "0x%x" % v
mixer = os.path.join(tmp, "mixer_%s_%d.json" % (mode, os.getpid()))
json.dump({k: hx(v) for k, v in random_mixer(random.Random(7)).items()}, open(mixer, "w"))
out = {"process_before": tkmk.root_generator()}
if mode == "single":
    with service.Prover(qap, crs, testing=True) as p:
        out["gen"] = p.root_generator
        out["proof"] = p.prove(synth, None, testing_mixer_json=mixer)[0]
elif mode == "sharded":
    comms = dist.loopback_comms(2)
    provers = dist.run_ranks(comms, lambda c: service.Prover(qap, crs, testing=True, comm=c))
    by_rank = {p.comm.rank: p for p in provers}
    out["gens"] = [by_rank[r].root_generator for r in range(2)]
    out["proofs"] = dist.run_ranks(comms, lambda c: by_rank[c.rank].prove(synth, None, testing_mixer_json=mixer)[0])
    for p in provers:
        p.close()
    for c in comms:
        c.close()
elif mode == "second":
    first = service.Prover(qap, crs, testing=True)
    out["gen"] = first.root_generator
    out["proof"] = first.prove(synth, None, testing_mixer_json=mixer)[0]
    try:
        service.Prover(qap, sys.argv[6], testing=True)
        out["second"] = "opened"
    except service.ProverError as e:
        out["second"] = [e.code, str(e)]
    out["proof_again"] = first.prove(synth, None, testing_mixer_json=mixer)[0]
    out["gen_again"] = first.root_generator
    first.close()
    with service.Prover(qap, sys.argv[6], testing=True) as p:             # the only context of the process now: adopted
        out["after_close"] = p.root_generator
elif mode == "domain":
    tkmk.init_ntt_domain_for_size(16)
    try:
        tkmk.set_root_generator(7)
        out["with_domain"] = "accepted"
    except tkmk.TkmkError as e:
        out["with_domain"] = e.code
    tkmk.set_root_generator(5)                                             # the generator in effect: always fine
    tkmk.release_ntt_domain()
    tkmk.set_root_generator(7)
    tkmk.init_ntt_domain_for_size(16)
    w = int.from_bytes(bytes(tkmk.get_root_of_unity(16)), "little")
    out["root"] = "0x%x" % w
out["process_after"] = tkmk.root_generator()
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def proof_under_the_override(world):
    out = _py(LIB_CODE, ["single", world.qap, world.synth, world.tmp, world.crs7], gen=7)
    assert out["gen"] == 7 and out["process_before"] == 7
    return out["proof"]


def test_library_adopts_and_proves_as_under_the_override(world, proof_under_the_override):
    out = _py(LIB_CODE, ["single", world.qap, world.synth, world.tmp, world.crs7])
    assert out["process_before"] == 5 and out["gen"] == 7 and out["process_after"] == 7
    assert out["proof"] == proof_under_the_override


def test_sharded_ranks_adopt_together(world, proof_under_the_override):
    out = _py(LIB_CODE, ["sharded", world.qap, world.synth, world.tmp, world.crs7])
    assert out["process_before"] == 5 and out["gens"] == [7, 7] and out["process_after"] == 7
    assert out["proofs"][0] == proof_under_the_override and out["proofs"][1] == proof_under_the_override


def test_a_switch_is_refused_while_another_context_is_open(world):
    out = _py(LIB_CODE, ["second", world.qap, world.synth, world.tmp, world.crs5, world.crs7])
    assert out["gen"] == 5
    code, msg = out["second"]
    assert code == 11 and "generator 7" in msg and "generator 5" in msg, msg
    assert out["proof_again"] == out["proof"] and out["gen_again"] == 5
    assert out["after_close"] == 7 and out["process_after"] == 7


def test_set_root_generator_is_refused_while_a_domain_is_initialised(world):
    out = _py(LIB_CODE, ["domain", world.qap, world.synth, world.tmp, world.crs5])
    assert out["with_domain"] == 11
    r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    w = pow(7, (r - 1) >> 32, r)
    for _ in range(28):
        w = w * w % r
    assert int(out["root"], 16) == w and out["process_after"] == 7
