"""gpu tier: tkmk_msm_segmented (csrc/msm_impl.inc: k_msm_segmented + k_msm_segmented_finish) — many ragged few-term MSMs over views and
index lists of one resident table in two launches, the tail on the device.

Every comparison is an equality of BYTES of the 144-byte canonical projective record: against oracle.g1_msm on the gathered operands
(turned into the record: (x, y, 1), or (0, 1, 0) for infinity), and against tkmk.msm_multi_ex on the same job list.  One exception to the
second checker, stated where it applies: tkmk_msm_multi_ex hands a ONE-term job to bls12_381_msm's single-term kernel, which does not
read cfg->bitsize, so under a bitsize below the scalar's width its result is not the masked sum; there the oracle alone decides."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TABLE = 600
INVALID_ARGUMENT = 11


def _record(aff):
    """oracle affine (96 bytes, all zero = infinity) -> the library's canonical projective record"""
    out = np.zeros(144, np.uint8)
    if aff.any():
        out[:96] = aff
        out[96] = 1
    else:
        out[48] = 1
    return out


def _want(o, sc, pts):
    """sum_i sc[i] * pts[i] as a record; sc (n, 32) and pts (n, 96) host arrays"""
    sc, pts = np.ascontiguousarray(sc).reshape(-1), np.ascontiguousarray(pts).reshape(-1)
    if sc.size == 0:
        return _record(np.zeros(96, np.uint8))
    return _record(np.asarray(o.g1_msm(sc, pts)))


def _masked(o, sc, bits):
    return o.to_bytes([v & ((1 << bits) - 1) for v in o.to_ints(sc.reshape(-1), 32)], 32).reshape(-1, 32)


def _mont_points(o, table):
    """ICICLE's Montgomery form: x * 2^384 mod p, (0, 0) stays infinity"""
    return np.asarray(o.to_bytes([(x << 384) % o.P_MOD for x in o.to_ints(table, 48)], 48))


class World:
    pass


@pytest.fixture(scope="module")
def world(gpu, oracle):
    w = World()
    w.tk, w.o = gpu, oracle
    w.table = np.asarray(oracle.g1_random_bases(41, TABLE)).reshape(TABLE, 96).copy()
    w.table[17] = 0                                                   # an infinity record inside the table
    w.d_table = gpu.DeviceBuffer.from_host(w.table.reshape(-1))
    w.scalars = np.asarray(oracle.fr_random(42, 6000)).reshape(-1, 32).copy()
    w.d_scalars = gpu.DeviceBuffer.from_host(w.scalars.reshape(-1))
    return w


def _index_jobs(w, sizes, rnd, d_table=None):
    """jobs of the given sizes over index lists (repeats allowed) into the table, their scalars at consecutive offsets of ONE scalar
    buffer -> (jobs, expected records)"""
    total = sum(sizes)
    idx = rnd.integers(0, TABLE, max(total, 1), dtype=np.uint32)
    d_idx = w.tk.DeviceBuffer.from_host(idx.view(np.uint8))
    jobs, want, at = [], [], 0
    for n in sizes:
        jobs.append(dict(scalars=w.d_scalars, scalar_offset=32 * at, bases=w.d_table if d_table is None else d_table, n=n, base_index=d_idx, index_offset=4 * at,
                         table_len=TABLE))
        want.append(_want(w.o, w.scalars[at:at + n], w.table[idx[at:at + n]]))
        at += n
    return jobs, np.concatenate(want)


def _check_both(w, jobs, want, **kw):
    got = w.tk.msm_segmented(jobs, **kw)
    assert got.size == want.size
    bad = [k for k in range(len(jobs)) if not (got[144 * k:144 * (k + 1)] == want[144 * k:144 * (k + 1)]).all()]
    assert not bad, ("segmented vs oracle", bad[:10], [jobs[k]["n"] for k in bad[:10]])
    multi = w.tk.msm_multi_ex(jobs, **{k: v for k, v in kw.items() if k in ("bases_form", "bitsize")})
    assert (got == multi).all(), "segmented vs msm_multi_ex"
    _check_device_tail(w, jobs, got, **kw)
    return got


def _check_device_tail(w, jobs, got, **kw):
    """a call of few jobs finishes on the host, a large or an asynchronous one in k_msm_segmented_finish: the same bytes from the kernel"""
    d_res = w.tk.msm_segmented(jobs, results_on_device=True, is_async=True, **kw)
    w.tk.msm_segmented_status()
    assert (d_res.to_host(144 * len(jobs)) == got).all(), "device tail vs host tail"


# ---------------------------------------------------------------------------------------------------------------- sizes
def test_ragged_sizes_in_one_call(world):
    """the empty job, no reduction, the slot boundary, a second and a third trip, the cap — in this mixed order, one call"""
    w = world
    jobs, want = _index_jobs(w, [0, 1, 2, 3, 63, 64, 65, 128, 129, 4096], np.random.default_rng(1))
    _check_both(w, jobs, want)


def test_a_single_one_term_job(world):
    w = world
    jobs, want = _index_jobs(w, [1], np.random.default_rng(2))
    _check_both(w, jobs, want)


def test_a_thousand_jobs_of_one_to_three_terms(world):
    w = world
    rnd = np.random.default_rng(3)
    jobs, want = _index_jobs(w, [int(v) for v in rnd.integers(1, 4, 1000)], rnd)
    _check_both(w, jobs, want)


# ---------------------------------------------------------------------------------------------------------------- addressing
@pytest.mark.parametrize("box", [(5, 7), (20, 9)])                     # 35 terms: one trip; 180: three
def test_addressing_modes_give_the_same_sums(world, box):
    """a tx x ty box of a 32 x 16 scalar matrix against the matching box of a 24 x 12 table, addressed five ways"""
    w, tk, o = world, world.tk, world.o
    tx, ty = box
    rows, cols, xs, ys = 24, 12, 32, 16
    table = w.table[:rows * cols]
    coeffs = w.scalars[:xs * ys]
    c = coeffs.reshape(xs, ys, 32)[:tx, :ty].reshape(-1, 32)
    b = table.reshape(rows, cols, 96)[:tx, :ty].reshape(-1, 96)
    want = _want(o, c, b)
    d_c, d_b = tk.DeviceBuffer.from_host(np.ascontiguousarray(c).reshape(-1)), tk.DeviceBuffer.from_host(np.ascontiguousarray(b).reshape(-1))
    box_idx = (np.arange(tx)[:, None] * cols + np.arange(ty)[None, :]).reshape(-1).astype(np.uint32)
    d_box_idx = tk.DeviceBuffer.from_host(box_idx.view(np.uint8))
    n = tx * ty
    jobs = [dict(scalars=d_c, bases=d_b, n=n),                                                                    # contiguous
            dict(scalars=d_c, bases=w.d_table, n=n, base_view=(ty, cols), table_len=rows * cols),                # strided bases, cols < stride
            dict(scalars=w.d_scalars, bases=d_b, n=n, scalar_view=(ty, ys)),                                      # strided scalars
            dict(scalars=w.d_scalars, bases=w.d_table, n=n, scalar_view=(ty, ys), base_view=(ty, cols), table_len=TABLE),
            dict(scalars=d_c, bases=w.d_table, n=n, base_index=d_box_idx, table_len=TABLE)]                       # index list
    _check_both(w, jobs, np.concatenate([want] * len(jobs)))
    # repeated indices, and two jobs that share one scalar buffer at different offsets
    rep = np.array([3, 3, 3, 9, 3, 9, 200, 200] * 9, np.uint32)[:70]
    d_rep = tk.DeviceBuffer.from_host(rep.view(np.uint8))
    jobs = [dict(scalars=w.d_scalars, scalar_offset=32 * 100, bases=w.d_table, n=70, base_index=d_rep, table_len=TABLE),
            dict(scalars=w.d_scalars, scalar_offset=32 * 135, bases=w.d_table, n=35, base_index=d_rep, index_offset=4 * 35, table_len=TABLE)]
    want2 = np.concatenate([_want(o, w.scalars[100:170], w.table[rep]), _want(o, w.scalars[135:170], w.table[rep[35:]])])
    _check_both(w, jobs, want2)
    # a box that does not fit its table is refused before anything is launched
    with pytest.raises(tk.TkmkError) as e:
        tk.msm_segmented([dict(scalars=w.d_scalars, bases=w.d_table, n=TABLE, base_view=(cols, cols + 1), table_len=TABLE)])
    assert e.value.code == INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------- forms
@pytest.mark.parametrize("form", ["plain", "montgomery", "converted", "montgomery_scalars"])
def test_base_and_scalar_forms(world, form):
    w, tk, o = world, world.tk, world.o
    kw = {}
    d_table = w.d_table
    if form == "montgomery":
        d_table, kw = tk.DeviceBuffer.from_host(_mont_points(o, w.table.reshape(-1))), dict(bases_form=tk.BASES_MONTGOMERY)
    elif form == "converted":
        d_table, kw = tk.msm_convert_bases(w.table.reshape(-1)), dict(bases_form=tk.BASES_CONVERTED)
    rnd = np.random.default_rng(4)
    jobs, want = _index_jobs(w, [1, 5, 70, 2], rnd, d_table=d_table)
    jobs[1]["base_index"] = tk.DeviceBuffer.from_host(np.array([17, 3, 17, 4, 5], np.uint32).view(np.uint8))     # infinity records in every form
    jobs[1]["index_offset"] = 0
    want[144:288] = _want(o, w.scalars[1:6], w.table[[17, 3, 17, 4, 5]])
    if form == "montgomery_scalars":
        mont = np.asarray(o.to_bytes([(v << 256) % o.R_MOD for v in o.to_ints(w.scalars.reshape(-1), 32)], 32))
        d_mont = tk.DeviceBuffer.from_host(mont)
        for j in jobs:
            j["scalars"] = d_mont
        got = tk.msm_segmented(jobs, scalars_montgomery=True)
        assert (got == want).all()
        _check_device_tail(w, jobs, got, scalars_montgomery=True)
        assert (got == tk.msm_segmented([dict(j, scalars=w.d_scalars) for j in jobs])).all()
    else:
        _check_both(w, jobs, want, **kw)


# ---------------------------------------------------------------------------------------------------------------- degenerate sums
def test_degenerate_sums(world):
    w, tk, o = world, world.tk, world.o
    s = w.scalars[7:8]
    p = w.table[5:6]
    neg = np.asarray(o.g1_neg(p.reshape(-1).copy())).reshape(1, 96)
    special = o.to_bytes([0, 1, o.R_MOD - 1, 0, 1, o.R_MOD - 1, 2, 15, 16], 32).reshape(-1, 32)
    cases = [(np.repeat(s, 64, 0), np.repeat(p, 64, 0)),                       # the same record with the same scalar 64 times: equal points at every level
             (np.repeat(s, 2, 0), np.concatenate([p, neg])),                   # s P + s (-P) = infinity
             (np.repeat(s, 6, 0), np.concatenate([p, neg] * 3)),
             (w.scalars[20:25], np.concatenate([w.table[17:18], w.table[30:31], np.zeros((1, 96), np.uint8), w.table[17:18], w.table[31:32]])),   # infinity records
             (w.scalars[20:22], np.zeros((2, 96), np.uint8)),                  # nothing but infinity
             (special, w.table[40:49]),                                        # the scalars 0, 1 and r - 1
             (special[2:3], p),                                                # (r - 1) P = -P, alone
             (np.zeros((70, 32), np.uint8), w.table[100:170]),                 # every scalar 0
             (np.repeat(special[1:2], 65, 0), np.repeat(p, 65, 0))]            # 65 P through two trips
    sc = np.concatenate([c[0] for c in cases])
    pts = np.concatenate([c[1] for c in cases])
    d_sc, d_pts = tk.DeviceBuffer.from_host(sc.reshape(-1)), tk.DeviceBuffer.from_host(pts.reshape(-1))
    jobs, want, at = [], [], 0
    for c in cases:
        n = len(c[0])
        jobs.append(dict(scalars=d_sc, scalar_offset=32 * at, bases=d_pts, base_offset=96 * at, n=n))
        want.append(_want(o, c[0], c[1]))
        at += n
    want = np.concatenate(want)
    got = _check_both(w, jobs, want)
    inf = _record(np.zeros(96, np.uint8))
    for k in (1, 2, 4, 7):
        assert (got[144 * k:144 * (k + 1)] == inf).all(), k                    # (0, 1, 0)
    assert (got[144 * 6:144 * 6 + 96] == neg.reshape(-1)).all()


# ---------------------------------------------------------------------------------------------------------------- bitsize
@pytest.mark.parametrize("bits", [1, 4, 5, 128, 255])
def test_bitsize_masks_the_scalars(world, bits):
    """128 is the batch verifier's weight width.  msm_multi_ex is compared on the jobs of two terms and more (module docstring)"""
    w, tk, o = world, world.tk, world.o
    rnd = np.random.default_rng(5)
    sizes = [1, 3, 70, 2, 1]
    jobs, _ = _index_jobs(w, sizes, rnd)
    idx = jobs[0]["base_index"].to_host().view(np.uint32)
    want, at = [], 0
    for n in sizes:
        want.append(_want(o, _masked(o, w.scalars[at:at + n], bits), w.table[idx[at:at + n]]))
        at += n
    want = np.concatenate(want)
    got = tk.msm_segmented(jobs, bitsize=bits)
    assert (got == want).all()
    _check_device_tail(w, jobs, got, bitsize=bits)
    many = [k for k, n in enumerate(sizes) if n >= 2]
    multi = tk.msm_multi_ex([jobs[k] for k in many], bitsize=bits)
    for a, k in enumerate(many):
        assert (multi[144 * a:144 * (a + 1)] == got[144 * k:144 * (k + 1)]).all(), k


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refused(tk, call):
    with pytest.raises(tk.TkmkError) as e:
        call()
    assert e.value.code == INVALID_ARGUMENT


def test_refusals(world):
    w, tk, o = world, world.tk, world.o
    idx = np.array([1, 2, 3, 599, 5, 6], np.uint32)
    bad = idx.copy()
    bad[3] = TABLE                                                     # equal to base_table_len
    d_idx, d_bad = tk.DeviceBuffer.from_host(idx.view(np.uint8)), tk.DeviceBuffer.from_host(bad.view(np.uint8))
    good = dict(scalars=w.d_scalars, bases=w.d_table, n=6, base_index=d_idx, table_len=TABLE)
    want = _want(o, w.scalars[:6], w.table[idx])
    _refused(tk, lambda: tk.msm_segmented([good, dict(good, base_index=d_bad)]))
    _refused(tk, lambda: tk.msm_segmented([good] * 40 + [dict(good, base_index=d_bad)]))            # a call large enough for the device tail
    _refused(tk, lambda: tk.msm_segmented([dict(good, base_index=d_bad, n=4, scalar_offset=32 * 64)], bitsize=4))   # flagged whatever the digits are
    assert (tk.msm_segmented([good, good]) == np.concatenate([want, want])).all()                   # the same buffers, still correct
    big = tk.DeviceBuffer.from_host(np.zeros(4 * 4097, np.uint8))
    assert tk.msm_segmented([dict(good, base_index=big, n=4096)]).size == 144
    _refused(tk, lambda: tk.msm_segmented([dict(good, base_index=big, n=4097)]))
    _refused(tk, lambda: tk.msm_segmented([good, dict(good, table=(8, 2))]))                        # table_c != 0
    _refused(tk, lambda: tk.msm_segmented([dict(good, table=(0, 2))]))
    _refused(tk, lambda: tk.msm_segmented([good], bases_form=tk.BASES_ACC_READY))
    _refused(tk, lambda: tk.msm_segmented([dict(good, table_len=0)]))                               # an index list without base_table_len
    _refused(tk, lambda: tk.msm_segmented([dict(good, n=1, table_len=0)]))
    # host operands: the binding always says "device", so the C entry is called with a config that does not
    cfg = tk.lib().tkmk_msm_default_config()
    arr = tk.msm_job_ex_array([good], count=False)
    out = np.empty(144, np.uint8)
    for on_s, on_p in ((False, True), (True, False), (False, False)):
        cfg.are_scalars_on_device, cfg.are_points_on_device = on_s, on_p
        assert tk.lib().tkmk_msm_segmented(arr, 1, ctypes.byref(cfg), tk.BASES_PLAIN, out.ctypes.data_as(ctypes.c_void_p)) == INVALID_ARGUMENT
    cfg.are_scalars_on_device = cfg.are_points_on_device = True
    cfg.batch_size = 2
    assert tk.lib().tkmk_msm_segmented(arr, 1, ctypes.byref(cfg), tk.BASES_PLAIN, out.ctypes.data_as(ctypes.c_void_p)) == INVALID_ARGUMENT
    assert (tk.msm_segmented([good]) == want).all()


# ---------------------------------------------------------------------------------------------------------------- device results, counters
def test_results_on_device_and_the_asynchronous_form(world):
    w, tk = world, world.tk
    jobs, want = _index_jobs(w, [1, 0, 66, 3], np.random.default_rng(6))
    d_res = tk.msm_segmented(jobs, results_on_device=True)
    assert (d_res.to_host(144 * len(jobs)) == want).all()
    stream = ctypes.c_void_p()
    assert tk.lib().tkmk_stream_create(ctypes.byref(stream)) == 0
    try:
        d_res = tk.msm_segmented(jobs, results_on_device=True, is_async=True, stream=stream)
        tk.msm_segmented_status(stream)                                # waits for the stream; nothing was out of range
        assert (d_res.to_host(144 * len(jobs)) == want).all()
        bad = tk.DeviceBuffer.from_host(np.array([5, TABLE + 7], np.uint32).view(np.uint8))
        tk.msm_segmented([dict(jobs[3], n=2, base_index=bad, index_offset=0)], results_on_device=True, is_async=True, stream=stream)
        _refused(tk, lambda: tk.msm_segmented_status(stream))         # reported once
        tk.msm_segmented_status(stream)
    finally:
        assert tk.lib().tkmk_stream_destroy(stream) == 0


def test_counters(world):
    w, tk = world, world.tk
    sizes = [0, 1, 9, 64, 200]
    jobs, want = _index_jobs(w, sizes, np.random.default_rng(7))
    before = tk.native_stats()
    assert (tk.msm_segmented(jobs) == want).all()
    after = tk.native_stats()
    assert after["msm.segmented_jobs"] - before["msm.segmented_jobs"] == len(sizes)
    assert after["msm.segmented_terms"] - before["msm.segmented_terms"] == sum(sizes)
    assert after["msm.points"] == before["msm.points"] and after["msm.calls"] == before["msm.calls"]
