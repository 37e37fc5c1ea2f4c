"""gpu tier: the native verifier at the end of the product's own pipeline.  The verifier itself is host code (host/tkmk_verify.hpp); what
needs the GPU here is everything in front of it: bin/trusted-setup, bin/preprocess, bin/prove and the resident prover.

  * trusted-setup -> preprocess -> prove -> verify, the four binaries in tokamak-cli's runtime layout under the argv it sends: `true`; the
    same proof through tkmk_prover_verify on an open context: true; a changed proof: `false` by both routes; one cross-check against the
    Python verifier tests/verify_files.py over sigma_verify.json;
  * a CRS written under root-of-unity generator 7: a default-configured process adopts 7 at open and its tkmk_prover_verify says true;
    bin/verify with nothing pinned says `false`, with TKMK_FR_ROOT_GENERATOR=7 `true` — the documented limitation (sigma_verify.json
    cannot tell its generator), pinned;
  * the reference's real 14-subcircuit library: one proof, `true`;
  * one proof of the loopback sharded prover (G = 2): true from tkmk_prover_verify on rank 0.
bin/verify always runs as a child process with its own timeout; nothing here loads a sanitizer."""
import json
import os
import random
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

from test_gpu_real_library import runtime  # noqa: F401  (the module-scoped fixture: the real library through the three binaries)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "tokamak-zk-evm_amd")
BIN = os.path.join(PKG, "bin")


def _env(gen=None, home=None):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG, HERE, os.path.join(ROOT, "tools")]))
    for k in ("TKMK_FR_ROOT_GENERATOR", "TKMK_HOST_TRACE", "TKMK_SUBCIRCUIT_LIBRARY", "XDG_CACHE_HOME"):
        env.pop(k, None)
    if gen is not None:
        env["TKMK_FR_ROOT_GENERATOR"] = str(gen)
    if home is not None:
        env["HOME"] = str(home)
    return env


def _verdict(cmd, env, timeout=60):
    """runs a `verify` binary -> (True / False from the last stdout line, stderr)"""
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (cmd, r.stdout, r.stderr)
    last = r.stdout.strip().split("\n")[-1]
    assert last in ("true", "false"), r.stdout
    return last == "true", r.stderr


def _verify_args(crs, synth, pre, proof):                                           # cli.ts:548-559 backendVerifyArgs, verbatim
    return ["--crs", str(crs), "--synthesizer-stat", str(synth), "--preprocess", str(pre), "--proof", str(proof)]


class Pipeline:
    pass


@pytest.fixture(scope="module")
def pipeline(gpu, tmp_path_factory):
    """tokamak-cli's runtime layout with all FOUR binaries, after trusted-setup -> preprocess -> prove under its argv"""
    import synth_circuit
    p = Pipeline()
    tmp = tmp_path_factory.mktemp("verify_pipeline")
    rt = tmp / "runtime"
    (rt / "bin").mkdir(parents=True)
    for name in ("trusted-setup", "preprocess", "prove", "verify"):
        shutil.copy(os.path.join(BIN, name), rt / "bin" / name)
    os.symlink(os.path.join(PKG, "libtkmk_hip.so"), rt / "libtkmk_hip.so")          # the three device binaries' rpath is $ORIGIN/..
    inst = synth_circuit.build(str(tmp / "work"), random.Random(91), s_max=8, n_gate_kinds=2, used_placements=8, bit_fraction=0.4)
    res = rt / "resource"
    shutil.copytree(inst["qap"], res / "qap-compiler" / "library")
    p.dirs = {k: res / k / "output" for k in ("setup", "synthesizer", "preprocess", "prove")}
    shutil.copytree(inst["synth"], p.dirs["synthesizer"])
    for k in ("setup", "preprocess", "prove"):
        p.dirs[k].mkdir(parents=True)
    p.env = _env(home=tmp / "home")                                                 # no library anywhere but next to the installation
    out_args = lambda out: ["--crs", str(p.dirs["setup"]), "--synthesizer-stat", str(p.dirs["synthesizer"]), "--output", str(out)]      # noqa: E731
    for cmd in ([str(rt / "bin" / "trusted-setup"), "--output", str(p.dirs["setup"]), "--fixed-tau"],
                [str(rt / "bin" / "preprocess")] + out_args(p.dirs["preprocess"]), [str(rt / "bin" / "prove")] + out_args(p.dirs["prove"])):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=p.env)
        assert r.returncode == 0, (cmd, r.stdout, r.stderr)
    p.tmp, p.rt, p.qap = tmp, rt, str(res / "qap-compiler" / "library")
    p.verify = [str(rt / "bin" / "verify")]
    return p


def _changed_proofs(p):
    """-> {name: directory} of proof.json variants that are still well formed: one byte of an evaluation flipped; Pi_X replaced by
    another valid point of the group (its negative)"""
    from tkmk import proofio
    import oracle
    doc = json.load(open(p.dirs["prove"] / "proof.json"))
    out = {}
    flipped = json.loads(json.dumps(doc))
    h = flipped["proof_entries_part2"][-4]                                           # R_eval
    flipped["proof_entries_part2"][-4] = h[:-1] + ("0" if h[-1] != "0" else "1")
    points, scalars = proofio.recover_proof(doc)
    negated = proofio.format_proof(dict(points, Pi_X=np.asarray(oracle.g1_neg(points["Pi_X"].copy()))), scalars)
    assert negated != doc
    for name, d in (("flipped", flipped), ("negated", negated)):
        out[name] = p.tmp / ("proof_" + name)
        out[name].mkdir(exist_ok=True)
        proofio.write_json(out[name] / "proof.json", d)
    return out


def test_pipeline_of_four_binaries_and_the_self_check_of_a_context(gpu, pipeline):
    from tkmk import service, verify
    p = pipeline
    d = p.dirs
    ok, err = _verdict(p.verify + _verify_args(d["setup"], d["synthesizer"], d["preprocess"], d["prove"]), p.env)
    assert ok, err
    changed = _changed_proofs(p)
    for name, proof_dir in changed.items():
        ok, err = _verdict(p.verify + _verify_args(d["setup"], d["synthesizer"], d["preprocess"], proof_dir), p.env)
        assert not ok and "pairing product != 1" in err, (name, err)
    with service.Prover(p.qap, str(d["setup"])) as ctx:
        ok, rep = verify.prover_verify(ctx, str(d["synthesizer"]), str(d["preprocess"]), str(d["prove"]))
        assert ok and rep["generator"] == ctx.root_generator, rep
        for name, proof_dir in changed.items():
            ok, rep = verify.prover_verify(ctx, str(d["synthesizer"]), str(d["preprocess"]), str(proof_dir))
            assert not ok and rep["reason"] == "pairing product != 1", (name, rep)
        # the context proves on after verifying, and verifies what it proved
        out = p.tmp / "resident"
        out.mkdir()
        ctx.prove(str(d["synthesizer"]), str(out), want_json=False)
        ok, rep = verify.prover_verify(ctx, str(d["synthesizer"]), str(d["preprocess"]), str(out))
        assert ok, rep
        # the files route names the same challenges for the same proof
        ok2, rep2 = verify.verify_files(p.qap, str(d["setup"]), str(d["synthesizer"]), str(d["preprocess"]), str(out))
        assert ok2 and {k: rep2[k] for k in ("thetas", "chi", "zeta", "kappa1", "a_eval")} == {k: rep[k] for k in ("thetas", "chi", "zeta", "kappa1", "a_eval")}


def test_pipeline_verdicts_equal_the_python_verifier(gpu, pipeline):
    """once: tests/verify_files.py over sigma_verify.json (10 Python pairings) on the files bin/verify said `true` for"""
    import verify_files
    p = pipeline
    d = p.dirs
    both = p.tmp / "prove_and_preprocess"
    both.mkdir()
    shutil.copy(d["prove"] / "proof.json", both / "proof.json")
    shutil.copy(d["preprocess"] / "preprocess.json", both / "preprocess.json")
    assert verify_files.verify(p.qap, str(d["synthesizer"]), str(d["setup"]), str(both), from_sigma_verify=True) is True
    assert _verdict(p.verify + _verify_args(d["setup"], d["synthesizer"], both, both), p.env)[0] is True


SELF_CHECK_CODE = """
import json, sys
import tkmk
from tkmk import service, verify
qap, crs, synth, pre, out = sys.argv[1:6]
tkmk.set_device(0)
before = tkmk.root_generator()
with service.Prover(qap, crs) as p:
    p.prove(synth, out, want_json=False)
    ok, rep = verify.prover_verify(p, synth, pre, out)
    print(json.dumps({"before": before, "context": p.root_generator, "ok": ok, "report": rep}))
"""


def test_crs_made_under_generator_7(gpu, tmp_path):
    """trusted-setup and preprocess run under TKMK_FR_ROOT_GENERATOR=7 (the way tests/test_root_convention.py makes such a CRS); everything
    after that runs with the variable removed unless stated"""
    import synth_circuit
    inst = synth_circuit.build(str(tmp_path), random.Random(81), s_max=8, n_gate_kinds=2, used_placements=8, bit_fraction=0.4)
    assert inst["setup_params"]["l_D"] - inst["setup_params"]["l"] > 2               # the two generators give different roots here
    crs, pre, out = tmp_path / "crs7", tmp_path / "pre7", tmp_path / "out"
    for d in (crs, pre, out):
        d.mkdir()
    r = subprocess.run([os.path.join(BIN, "trusted-setup"), "--fixed-tau", "--subcircuit-library", inst["qap"], "--output", str(crs)],
                       capture_output=True, text=True, timeout=600, env=_env(7))
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(BIN, "preprocess"), "--crs", str(crs), "--synthesizer-stat", inst["synth"], "--output", str(pre), "--subcircuit-library", inst["qap"]],
                       capture_output=True, text=True, timeout=600, env=_env(7))
    assert r.returncode == 0, r.stderr
    # a default-configured process: the context adopts 7 from the CRS and verifies its own proof with no environment set
    r = subprocess.run([sys.executable, "-c", SELF_CHECK_CODE, inst["qap"], str(crs), inst["synth"], str(pre), str(out)],
                       capture_output=True, text=True, timeout=600, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["before"] == 5 and got["context"] == 7 and got["ok"] is True and got["report"]["generator"] == 7, got
    # bin/verify has sigma_verify.json only, which cannot tell: nothing pinned -> the declared default -> false; pinned to 7 -> true
    argv = [os.path.join(BIN, "verify")] + _verify_args(crs, inst["synth"], pre, out) + ["--subcircuit-library", inst["qap"]]
    ok, err = _verdict(argv, _env())
    assert not ok and "generator 5" in err and "pairing product != 1" in err, err
    ok, err = _verdict(argv, _env(7))
    assert ok and "generator 7" in err, err
    ok, err = _verdict(argv, _env(5))
    assert not ok, err


def test_real_library_proof_verifies(gpu, runtime):  # noqa: F811
    """the reference's real 14-subcircuit library in tokamak-cli's runtime layout: bin/verify next to the other three, the CLI's argv"""
    d = runtime["dirs"]
    rt_bin = os.path.join(runtime["tmp"], "runtime", "bin")
    shutil.copy(os.path.join(BIN, "verify"), os.path.join(rt_bin, "verify"))
    t = time.perf_counter()
    ok, err = _verdict([os.path.join(rt_bin, "verify")] + _verify_args(d["setup"], d["synthesizer"], d["preprocess"], d["prove"]), _env(home=os.path.join(runtime["tmp"], "home")))
    wall = time.perf_counter() - t
    print("bin/verify on the real library: %.3f s from process start to the verdict" % wall)
    assert ok, err
    ins = json.load(open(os.path.join(d["synthesizer"], "instance.json")))
    ins["a_pub_user"][0] = hex(int(ins["a_pub_user"][0], 16) ^ 1)
    other = os.path.join(runtime["tmp"], "synth_changed")
    os.makedirs(other, exist_ok=True)
    json.dump(ins, open(os.path.join(other, "instance.json"), "w"))
    ok, err = _verdict([os.path.join(rt_bin, "verify")] + _verify_args(d["setup"], other, d["preprocess"], d["prove"]), _env(home=os.path.join(runtime["tmp"], "home")))
    assert not ok and "pairing product != 1" in err, err


def test_sharded_prover_proof_verifies_on_rank_0(gpu, oracle, tmp_path):
    """one small-shape proof of the loopback sharded prover (G = 2): every rank holds the CRS's single points, no collective is involved"""
    import synth_circuit
    from test_gpu_prove import _stage_crs_file
    from tkmk import dist, service, verify
    inst = synth_circuit.build(str(tmp_path), random.Random(67), s_max=8, n_gate_kinds=2, used_placements=7, bit_fraction=0.4)
    crs_dir, out = str(tmp_path / "crs"), str(tmp_path / "out")
    _stage_crs_file(gpu, oracle, inst, crs_dir)
    os.makedirs(out)
    r = subprocess.run([os.path.join(BIN, "preprocess"), "--crs", crs_dir, "--synthesizer-stat", inst["synth"], "--output", out, "--subcircuit-library", inst["qap"]],
                       capture_output=True, text=True, timeout=600, env=_env())
    assert r.returncode == 0, r.stderr
    comms = dist.loopback_comms(2)
    provers = dist.run_ranks(comms, lambda c: service.Prover(inst["qap"], crs_dir, testing=True, comm=c))
    by_rank = {p.comm.rank: p for p in provers}
    try:
        dist.run_ranks(comms, lambda c: by_rank[c.rank].prove(inst["synth"], out)[0])
        ok, rep = verify.prover_verify(by_rank[0], inst["synth"], out, out)          # rank 0 alone: nothing to meet its peers for
        assert ok, rep
        ok, rep = verify.prover_verify(by_rank[1], inst["synth"], out, out)
        assert ok, rep
    finally:
        for p in provers:
            p.close()
        for c in comms:
            c.close()
