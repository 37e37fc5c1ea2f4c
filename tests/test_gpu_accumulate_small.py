"""gpu tier: the bucket accumulation (csrc/msm_impl.inc: k_accumulate_chunks_rows / k_accumulate_chunks, the mixed addition of
csrc/ec_u.h on the products of csrc/ffu.h) end to end at the smallest sizes that take each kernel: a table-mode MSM of 2^18 points at
c = 20 over accumulate-ready rows (the smallest the two-pass sort takes) and a plain 2^12-point MSM at c = 16 over 96-byte records,
both against the oracle.  The scalars make both signs of the signed digits, zero digits and a base repeated in its bucket (P + P: the
degenerate path through the saturated adder) all occur."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bases(oracle, seed, n, distinct):
    """`distinct` random points tiled to n, one infinity record, and neighbours that are the same point"""
    t = np.asarray(oracle.g1_random_bases(seed, distinct)).reshape(-1, 96)
    t = np.ascontiguousarray(np.tile(t, (n // distinct, 1)))
    t[7] = 0
    for i in range(32, n, n // 16):
        t[i + 1] = t[i]
    return t


def _scalars(seed, n):
    """uniform below 2^254 (all windows busy, both signs), with runs of: zero, below 2^20 (one busy window at c = 20), a zero window in
    the middle, all-ones windows (digit 2^c - 1: negative with a carry), and equal scalars on the repeated neighbours of _bases"""
    rnd = np.random.default_rng(seed)
    s = rnd.integers(0, 256, (n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3f
    k = n // 8
    s[0:k:5] = 0
    s[k:2 * k:3, 3:] = 0
    s[k:2 * k:3, 2] &= 0x0f
    s[2 * k:3 * k:2, 5:10] = 0
    s[3 * k:4 * k:4, 0:8] = 0xff
    for i in range(32, n, n // 16):
        s[i + 1] = s[i]
    return s


def _digits_seen(s, c):
    """the signed c-bit digits of the scalars (digit > 2^(c-1) -> digit - 2^c with a carry): which kinds occur"""
    neg = pos = zero = 0
    for row in s[:: max(1, s.shape[0] // 512)]:
        v, carry = int.from_bytes(row.tobytes(), "little"), 0
        for _ in range(255 // c + 1):
            d = (v & ((1 << c) - 1)) + carry
            v >>= c
            carry = 1 if d > (1 << (c - 1)) else 0
            neg, pos, zero = neg + (carry == 1), pos + (0 < d <= (1 << (c - 1))), zero + (d == 0)
    return neg, pos, zero


def test_table_mode_2p18_points_at_c20_matches_the_oracle(gpu, oracle):
    tk = gpu
    n, c, windows = 1 << 18, 20, 13
    bases = _bases(oracle, 0xACC1, n, 4096)
    s = _scalars(0xACC2, n)
    assert all(x > 0 for x in _digits_seen(s, c))
    d_rows = tk.msm_precompute_bases_acc(bases.reshape(-1), n, windows, c=c)
    d_sc = tk.DeviceBuffer.from_host(s.reshape(-1))
    got = tk.projective_to_affine_bytes(tk.msm_multi_ex([dict(scalars=d_sc, bases=d_rows, n=n, table_len=n, table=(c, windows))], bases_form=tk.BASES_ACC_READY))
    want = np.asarray(oracle.g1_msm(s.reshape(-1), bases.reshape(-1)))
    assert (got == want).all()


def test_plain_2p12_points_at_c16_matches_the_oracle(gpu, oracle):
    tk = gpu
    n, c = 1 << 12, 16
    bases = _bases(oracle, 0xACC3, n, 1024)
    s = _scalars(0xACC4, n)
    assert all(x > 0 for x in _digits_seen(s, c))
    got = tk.projective_to_affine_bytes(tk.msm(s.reshape(-1), bases.reshape(-1), c=c))
    want = np.asarray(oracle.g1_msm(s.reshape(-1), bases.reshape(-1)))
    assert (got == want).all()
