"""gpu tier: table jobs of tkmk_msm_multi_ex over ACCUMULATE-READY tables (bls12_381_msm_precompute_bases_acc, TKMK_BASES_ACC_READY:
128-byte rows on 128-byte lines, the form the resident prover holds its commit tables in) are bit-identical to the oracle's MSM and to
the same jobs over the 96-byte table under TKMK_BASES_CONVERTED; the form is decided per job, so one call may mix table jobs with
jobs over 96-byte converted records; a table pointer off its line is refused."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, COLS = 160, 256          # the grid: 40960 rows per table level
N = 1 << 15                    # contiguous jobs run over the first 2^15 rows: 2^15 x 13 levels >= 2^18 entries
BOX = (140, 240)               # a box strictly inside the grid: base_cols < base_stride, 33600 points
INVALID_ARGUMENT = 11


def _aff(tkmk, proj):
    return tkmk.projective_to_affine_bytes(proj)


def _table(oracle, seed):
    """4096 distinct points, tiled over the grid, with (0, 0) infinity rows at the first row, the last row of the contiguous jobs, the
    last row of the grid and at random positions"""
    t = np.asarray(oracle.g1_random_bases(seed, 4096))
    t = np.ascontiguousarray(np.tile(t.reshape(-1, 96), (ROWS * COLS // 4096, 1)))
    rnd = np.random.default_rng(seed)
    for i in [0, N - 1, ROWS * COLS - 1] + list(rnd.integers(1, ROWS * COLS - 1, 40)):
        t[i] = 0
    return t.reshape(-1)


def _scalars(oracle, kind, seed):
    s = np.asarray(oracle.fr_random(seed, 1 << 13))
    s = np.ascontiguousarray(np.tile(s.reshape(-1, 32), (ROWS * COLS // (1 << 13), 1)))
    if kind == "equal":                       # one giant bucket per level
        s[:] = s[5]
    elif kind == "small":                     # 30 % zeros, the rest below 2^20
        s[:, 3:] = 0
        s[:, 2] &= 0x0f
        s[np.random.default_rng(seed).random(s.shape[0]) < 0.3] = 0
    return s.reshape(-1)


@pytest.mark.parametrize("c", [16, 20])
def test_acc_ready_table_jobs_match_the_oracle_and_the_96_byte_table(gpu, oracle, c):
    tk = gpu
    windows = 255 // c + 1
    table = _table(oracle, 900 + c)
    d_rows = tk.msm_precompute_bases_acc(table, ROWS * COLS, windows, c=c)
    assert d_rows.nbytes == 128 * ROWS * COLS * windows and d_rows.ptr % 128 == 0
    d_96 = tk.msm_precompute_bases(table, ROWS * COLS, windows, c=c)
    tx, ty = BOX
    for kind in ("dense", "equal", "small"):
        sc = _scalars(oracle, kind, 910 + c)
        d_sc = tk.DeviceBuffer.from_host(sc)
        want = [np.asarray(oracle.g1_msm(np.ascontiguousarray(sc[:32 * N]), np.ascontiguousarray(table[:96 * N]))),
                np.asarray(oracle.g1_msm(np.ascontiguousarray(sc.reshape(ROWS, COLS, 32)[:tx, :ty].reshape(-1)),
                                         np.ascontiguousarray(table.reshape(ROWS, COLS, 96)[:tx, :ty].reshape(-1))))]

        def jobs(bases):
            return [dict(scalars=d_sc, bases=bases, n=N, table_len=ROWS * COLS, table=(c, windows)),
                    dict(scalars=d_sc, bases=bases, n=tx * ty, scalar_view=(ty, COLS), base_view=(ty, COLS), table_len=ROWS * COLS, table=(c, windows))]
        got = _aff(tk, tk.msm_multi_ex(jobs(d_rows), bases_form=tk.BASES_ACC_READY))
        got96 = _aff(tk, tk.msm_multi_ex(jobs(d_96), bases_form=tk.BASES_CONVERTED))
        for k, w in enumerate(want):
            assert (got[96 * k:96 * (k + 1)] == w).all(), (c, kind, k)
        assert (got == got96).all(), (c, kind)


def test_acc_ready_is_decided_per_job(gpu, oracle):
    """one call under BASES_ACC_READY: a table job over 128-byte rows, a table_c == 0 job over the 96-byte level 0, a base_index job
    over a 96-byte converted table — each returns its own oracle result"""
    tk = gpu
    c, windows = 20, 13
    table = _table(oracle, 930)
    d_rows = tk.msm_precompute_bases_acc(table, ROWS * COLS, windows, c=c)
    d_level0 = tk.msm_convert_bases(table)
    other = np.asarray(oracle.g1_random_bases(931, 5000))
    other[96 * 3:96 * 4] = 0
    d_other = tk.msm_convert_bases(other)
    sc = _scalars(oracle, "dense", 932)
    d_sc = tk.DeviceBuffer.from_host(sc)
    idx = np.random.default_rng(933).integers(0, 5000, 3000, dtype=np.uint32)
    d_idx = tk.DeviceBuffer.from_host(idx.view(np.uint8))
    jobs = [dict(scalars=d_sc, bases=d_rows, n=N, table_len=ROWS * COLS, table=(c, windows)),
            dict(scalars=d_sc, bases=d_level0, n=30 * 10, scalar_view=(10, COLS), base_view=(10, COLS), table_len=ROWS * COLS),
            dict(scalars=d_sc, bases=d_other, n=idx.size, base_index=d_idx, table_len=5000)]
    want = [oracle.g1_msm(np.ascontiguousarray(sc[:32 * N]), np.ascontiguousarray(table[:96 * N])),
            oracle.g1_msm(np.ascontiguousarray(sc.reshape(ROWS, COLS, 32)[:30, :10].reshape(-1)), np.ascontiguousarray(table.reshape(ROWS, COLS, 96)[:30, :10].reshape(-1))),
            oracle.g1_msm(np.ascontiguousarray(sc[:32 * idx.size]), np.ascontiguousarray(other.reshape(-1, 96)[idx].reshape(-1)))]
    got = _aff(tk, tk.msm_multi_ex(jobs, bases_form=tk.BASES_ACC_READY))
    for k, w in enumerate(want):
        assert (got[96 * k:96 * (k + 1)] == np.asarray(w)).all(), k


def test_acc_ready_table_off_its_line_is_refused(gpu, oracle):
    tk = gpu
    c, windows = 20, 13
    table = _table(oracle, 940)
    d_rows = tk.msm_precompute_bases_acc(table, ROWS * COLS, windows, c=c)
    d_sc = tk.DeviceBuffer.from_host(_scalars(oracle, "dense", 941))
    for off in (4, 64, 96):
        with pytest.raises(tk.TkmkError) as e:
            tk.msm_multi_ex([dict(scalars=d_sc, bases=d_rows, base_offset=off, n=N, table_len=ROWS * COLS, table=(c, windows))], bases_form=tk.BASES_ACC_READY)
        assert e.value.code == INVALID_ARGUMENT
    # a job with table_c > 0 is a table job over rows: a one-level table (table_factor 1) is refused, not read as 96-byte records
    with pytest.raises(tk.TkmkError) as e:
        tk.msm_multi_ex([dict(scalars=d_sc, bases=d_rows, n=N, table_len=ROWS * COLS, table=(c, 1))], bases_form=tk.BASES_ACC_READY)
    assert e.value.code == INVALID_ARGUMENT
    # and the table maker itself refuses an output that is not on a line start
    import ctypes
    cfg = tk.lib().tkmk_msm_default_config()
    cfg.precompute_factor, cfg.c = windows, c
    cfg.are_results_on_device = True
    rc = tk.lib().bls12_381_msm_precompute_bases_acc(table.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(ROWS * COLS), ctypes.byref(cfg),
                                                   ctypes.c_void_p(d_rows.ptr + 64), None)
    assert rc == INVALID_ARGUMENT
