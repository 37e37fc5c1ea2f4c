"""gpu tier: CommitBatch (tokamak-zk-evm_amd/host/tkmk_host.hpp) owns the operands it cuts.  Two loopback ranks each commit ONE batch
[P, P, Q, S] of replicated polynomials (tests/host_cpp/commit_batch_driver.cpp): the same polynomial twice in a batch (each job keeps its
own slice), a second polynomial, and a 4 x 1 one whose box leaves rank 1 without a column — in line, and again from the helper thread of
CommitBatch::start.  Every result is the world-1 commitment over the whole grid and [p(tau_x, tau_y)] G of the oracle."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "host_cpp", "commit_batch_driver")


def _records(path):
    raw = open(path, "rb").read()
    out, off = {}, 0
    while off < len(raw):
        tag, n = struct.unpack_from("<IQ", raw, off)
        off += 12
        out[tag] = np.frombuffer(raw[off:off + n], np.uint8).reshape(-1, 96)
        off += n
    return out


def test_batch_owns_its_slices_on_two_loopback_ranks(gpu, oracle, tmp_path):
    pins = json.load(open(os.path.join(HERE, "golden", "pins.json")))
    R = oracle.R_MOD
    rs_x = rs_y = 8
    shapes = [(4, 4), (2, 8), (4, 1)]                     # P, Q, S
    polys = [oracle.fr_random(31 + k, xs * ys) for k, (xs, ys) in enumerate(shapes)]
    for c, (xs, ys) in zip(polys, shapes):                # full boxes: the top coefficient is there (P: degree (3, 3))
        assert c[-32:].any()
    tx, ty = int(pins["tau_x"], 16), int(pins["tau_y"], 16)
    g = oracle.to_bytes([int(pins["fixed_tau_g1_x"], 16), int(pins["fixed_tau_g1_y"], 16)], 48)
    mon = [pow(tx, i, R) * pow(ty, j, R) % R for i in range(rs_x) for j in range(rs_y)]
    crs = gpu.g1_batch_scalar_mul_device(gpu.DeviceBuffer.from_host(oracle.to_bytes(mon, 32)), g, rs_x * rs_y).to_host()
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<8I", rs_x, rs_y, *[d for s in shapes for d in s]))
        for arr in [crs] + polys:
            f.write(arr.tobytes())
    gpu.release_scratch()
    subprocess.run([DRIVER, str(inp), str(outp)], check=True, timeout=120)
    rec = _records(outp)

    tau = oracle.to_bytes([tx], 32), oracle.to_bytes([ty], 32)
    want = [oracle.g1_scalar_mul(oracle.poly_eval(c, xs, ys, *tau), g) for c, (xs, ys) in zip(polys, shapes)]
    one_gpu = rec[1]
    assert one_gpu.shape == (3, 96)
    for k in range(3):
        assert (one_gpu[k] == want[k]).all()
    batch = [0, 0, 1, 2]                                  # [P, P, Q, S]
    for tag in (10, 11, 20, 21):                          # in line on rank 0, 1; through the helper-thread handle on rank 0, 1
        got = rec[tag]
        assert got.shape == (4, 96), tag
        assert (got[0] == got[1]).all(), tag              # the two jobs over P
        for j, k in enumerate(batch):
            assert (got[j] == one_gpu[k]).all(), (tag, j)
            assert (got[j] == want[k]).all(), (tag, j)
