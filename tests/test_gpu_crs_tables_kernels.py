"""gpu tier: the two kernels of csrc/crsaudit.hip, each on its own through the C ABI, against Python big integers.

  tkmk_fr_outer           out[j * out_stride + i] = col[j] * row[i]; the padding of a wider out_stride is not touched
  tkmk_r1cs_library_mix   u[c * out_stride + g] = sum over kinds and over the entries of row c of A whose wire routes to column g of
                          coeff * weight[kind][wire] (v, w from B, C), on hand-made libraries of 2 and 3 kinds
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _fr(vals):
    return np.frombuffer(b"".join(int(v % R).to_bytes(32, "little") for v in vals), np.uint8).copy() if len(vals) else np.zeros(0, np.uint8)


def _ints(buf):
    b = bytes(np.asarray(buf, np.uint8))
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]


def _vals(count, salt):
    """0, 1, r - 1 first, then values spread over the field"""
    special = [0, 1, R - 1]
    return [special[k] if k < 3 else pow(7 + salt, 1000 + 37 * k, R) for k in range(count)]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (8, 8)])
def test_fr_outer_vs_big_integers(gpu, rows, cols, pad):
    tk = gpu
    col, row = _vals(rows, 1), _vals(cols, 2)
    if rows == 1:
        col, row = [R - 1], [R - 1]                                    # (r - 1)^2 = 1
    stride = cols + pad
    fill = [0xABCDEF0000 + k for k in range(rows * stride)]
    out = tk.DeviceBuffer.from_host(_fr(fill))
    tk.fr_outer(tk.DeviceBuffer.from_host(_fr(col)), rows, tk.DeviceBuffer.from_host(_fr(row)), cols, out_stride=stride, out=out)
    tk.synchronize()
    got = _ints(out.to_host())
    want = list(fill)
    for j in range(rows):
        for i in range(cols):
            want[j * stride + i] = col[j] * row[i] % R
    assert got == want
    if rows == 1:
        assert got[0] == 1


def test_fr_outer_refuses_a_stride_below_cols(gpu):
    tk = gpu
    d = tk.DeviceBuffer.from_host(_fr(_vals(4, 3)))
    with pytest.raises(tk.TkmkError):
        tk.fr_outer(d, 2, d, 4, out_stride=3, out=tk.DeviceBuffer(32 * 8))


# ---- hand-made libraries: per kind (n_rows, n_wires, [A, B, C]) with a matrix = {row: [(wire, coeff)]} ----
def _kinds(n):
    k0 = (n, 5, [{0: [(0, 3), (4, R - 1)], 1: [(1, 1)], n - 1: [(2, 5), (3, 7), (0, 11)]},          # row 2 of A is empty
                 {0: [(4, 2)], 2: [(3, R - 2), (1, 9)]},
                 {}])                                                                                # C is an empty matrix
    k1 = (n - 1, 3, [{0: [(2, 13)], n - 2: [(0, 17), (1, 19)]},                                      # one row shorter than n
                     {1: [(1, 23)]},
                     {0: [(0, 29), (1, 31), (2, 37)], n - 2: [(2, 41)]}])
    k2 = (2, 7, [{1: [(6, 43), (5, 47)]},
                 {0: [(0, 53)], 1: [(3, 59), (4, 61)]},
                 {1: [(2, 67)]}])
    return [k0, k1, k2]


def _csr(n_rows, mat):
    ptr, wires, coeffs = [0], [], []
    for r in range(n_rows):
        for w, c in mat.get(r, []):
            wires.append(w)
            coeffs.append(c)
        ptr.append(len(wires))
    return np.asarray(ptr, np.uint32), np.asarray(wires, np.uint32), _fr(coeffs)


def _library(tk, kinds):
    from tkmk import witness
    return witness.R1csLibrary([tuple(_csr(nr, m) for m in mats) for nr, _, mats in kinds], [k[0] for k in kinds], [k[1] for k in kinds])


def _weights(kinds):
    out = []
    for s, (_, nw, _) in enumerate(kinds):
        w = _vals(nw, 10 + s)                                          # holds a wire with weight 0, one with 1, one with r - 1
        out.append(w)
    return out


def _want(kinds, weights, cols, n, n_cols, stride, fill):
    outs = [list(fill) for _ in range(3)]
    for m in range(3):
        for c in range(n):
            for g in range(n_cols):
                acc = 0
                for s, (nr, _, mats) in enumerate(kinds):
                    if c >= nr:
                        continue
                    for w, coeff in mats[m].get(c, []):
                        if (cols[s][w] if cols is not None and cols[s] is not None else 0) == g:
                            acc += coeff * weights[s][w]
                outs[m][c * stride + g] = acc % R
    return outs


def _run_mix(tk, kinds, cols, n, n_cols, stride):
    lib = _library(tk, kinds)
    weights = _weights(kinds)
    d_w = [tk.DeviceBuffer.from_host(_fr(w)) for w in weights]
    d_c = None if cols is None else [None if c is None else tk.DeviceBuffer.from_host(np.asarray(c, np.uint8)) for c in cols]
    fill = [0x5150000 + k for k in range(n * stride)]
    outs = [tk.DeviceBuffer.from_host(_fr(fill)) for _ in range(3)]
    try:
        tk.r1cs_library_mix(lib, d_w, d_c, n, n_cols, out_stride=stride, outs=outs)
        tk.synchronize()
        got = [_ints(o.to_host()) for o in outs]
    finally:
        lib.close()
    return got, _want(kinds, weights, cols, n, n_cols, stride, fill)


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("n,n_kinds", [(4, 2), (8, 3)])
def test_library_mix_one_column_without_a_column_map(gpu, n, n_kinds, stride):
    kinds = _kinds(n)[:n_kinds]
    got, want = _run_mix(gpu, kinds, None, n, 1, stride)
    assert got == want
    assert any(want[0][c * stride] for c in range(n))                  # not zeros against zeros


@pytest.mark.parametrize("stride", [4, 6])
@pytest.mark.parametrize("n,n_kinds", [(4, 2), (8, 3)])
def test_library_mix_routes_wires_to_four_columns(gpu, n, n_kinds, stride):
    kinds = _kinds(n)[:n_kinds]
    # columns 0, 1 and 3 are used, column 2 by no wire: it must come out zero; the last kind has no map (all of it to column 0)
    cols = [[0, 1, 3, 1, 0], [3, 0, 1], None][:n_kinds]
    got, want = _run_mix(gpu, kinds, cols, n, 4, stride)
    assert got == want
    for m in range(3):
        assert all(got[m][c * stride + 2] == 0 for c in range(n))
    assert any(got[0][c * stride + 3] for c in range(n)) and any(got[0][c * stride + 1] for c in range(n))


def test_library_mix_refusals(gpu):
    tk = gpu
    kinds = _kinds(4)[:2]
    with pytest.raises(tk.TkmkError):                                  # a column value >= n_cols
        _run_mix(tk, kinds, [[0, 1, 4, 1, 0], [3, 0, 1]], 4, 4, 4)
    with pytest.raises(tk.TkmkError):                                  # n_cols > out_stride
        _run_mix(tk, kinds, None, 4, 2, 1)
    with pytest.raises(tk.TkmkError):                                  # a kind with more rows than n
        _run_mix(tk, kinds, None, 2, 1, 1)
