"""gpu tier: one rank is G = 1 of the one code path (host/tkmk_witness_check.hpp run).  For EVERY case of
tests/test_gpu_witness_check_sharded.py — its documents, its single-GPU report as the reference — the collective entry
(tkmk_prover_check_witness_sharded) gives that report key for key outside "seconds" in both forms a world of one takes: a context from
tkmk_prover_open, which has no communicator, and the one rank of a one-rank loopback communicator.  Neither exchanges anything."""
import pytest

from test_gpu_witness_check_sharded import CASES, _without_seconds, documents, world   # noqa: F401  (the two fixtures, made once more for this module)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def alone(world):
    """the one rank of a one-rank communicator, open for the module"""
    from tkmk import dist, service
    comms = dist.loopback_comms(1)
    try:
        with service.Prover(world.qap, world.crs, testing=True, comm=comms[0]) as p:
            yield p
    finally:
        comms[0].close()


@pytest.mark.parametrize("name", CASES)
def test_world_of_one_is_the_unsharded_entry_in_every_case(world, alone, name):
    from tkmk import verify
    ok, rep = world.single_report(name)
    for prover in (world.single, alone):
        ok1, rep1 = verify.witness_check(None, world.cases[name]["synth"], prover=prover, collective=True)
        assert ok1 == ok and _without_seconds(rep1) == _without_seconds(rep), (name, prover is alone)
