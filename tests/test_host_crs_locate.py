"""not-gpu tier: the search of the CRS audit's locate pass (host/tkmk_crs_locate.hpp) through tests/host_cpp/crs_locate_driver, which has no
device, pairing or field dependency, and the public surface of the pass: tkmk_crs_audit_files_ex with its two flags in the header and the
library, `crs-check --locate` in the usage.  The search is run against a fake predicate — a range fails iff it meets a set of bad indices
— for every extent up to 33 and every bad set of one or two indices plus "all bad": the answer must be the first bad index, in at most
ceil(log2 n) + 1 predicate calls; the same for the rows-then-columns search up to 5 x 9.  The driver refuses (exit 1) a predicate call
over an empty range, past the extent or over the whole extent, so those are checked with every case."""
import ctypes
import itertools
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DRIVER = os.path.join(HERE, "host_cpp", "crs_locate_driver")
CRS_CHECK = os.path.join(ROOT, "tokamak-zk-evm_amd", "bin", "crs-check")


def _ceil_log2(n):
    return (n - 1).bit_length()


def _drive(lines):
    r = subprocess.run([DRIVER], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _bad_sets(universe):
    universe = list(universe)
    for k in (1, 2):
        yield from itertools.combinations(universe, k)
    yield tuple(universe)


def test_first_bad_index_of_every_extent_to_33():
    cases = [(n, bad) for n in range(1, 34) for bad in _bad_sets(range(n))]
    got = _drive(["1 %d %d %s" % (n, len(bad), " ".join(map(str, bad))) for n, bad in cases])
    assert len(cases) > 6000
    for (n, bad), (at, calls) in zip(cases, got):
        assert at == min(bad), (n, bad, at)
        assert calls <= _ceil_log2(n) + 1, (n, bad, calls)
    assert max(calls for _, calls in got) == _ceil_log2(33)       # the search itself never needs the + 1


def test_first_bad_cell_rows_then_columns_to_5_by_9():
    cases = [(rows, cols, bad) for rows in range(1, 6) for cols in range(1, 10)
             for bad in _bad_sets(itertools.product(range(rows), range(cols)))]
    got = _drive(["2 %d %d %d %s" % (rows, cols, len(bad), " ".join("%d %d" % c for c in bad)) for rows, cols, bad in cases])
    assert any(rows == 5 and cols == 9 for rows, cols, _ in cases) and any(rows == 3 and cols == 7 for rows, cols, _ in cases)
    for (rows, cols, bad), (r, c, calls) in zip(cases, got):
        assert (r, c) == min(bad), (rows, cols, bad, r, c)            # the first bad row, and its first bad column: row-major order
        assert calls <= _ceil_log2(rows) + _ceil_log2(cols) + 1, (rows, cols, bad, calls)


def test_the_driver_refuses_a_malformed_case():
    r = subprocess.run([DRIVER], input="1 0 0\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "extent" in r.stderr


def test_the_record_two_first_failing_relations_share():
    """record (a, b) of a table with rs_y = 16 records per row is wrong: the first failing relation along Y has it as target (source
    (a, b - 1)) unless b = 0, along X likewise (source (a - 1, b)) unless a = 0"""
    rs_y, rs_x = 16, 12
    cases, want = [], []
    for a, b in itertools.product(range(rs_x), range(rs_y)):
        if (a, b) == (0, 0):
            continue
        y = a * rs_y + (b - 1 if b else b)
        x = (a - 1 if a else a) * rs_y + b
        cases.append("3 %d %d %d" % (y, x, rs_y))
        want.append((a * rs_y + b,))
    cases.append("3 %d %d %d" % (5, 5 + 3 * rs_y, rs_y))       # two relations far apart: no record in common
    want.append((-1,))
    assert _drive(cases) == want


def test_header_declares_and_library_exports_the_flagged_entry():
    hdr = open(os.path.join(ROOT, "include", "tkmk_prover.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+TKMK_CRS_AUDIT_CIRCUIT\s+1\b", code) and re.search(r"#define\s+TKMK_CRS_AUDIT_LOCATE\s+2\b", code)
    assert re.search(r"tkmk_error\s+tkmk_crs_audit_files_ex\s*\(\s*const char \*\w+,\s*const char \*\w+,\s*(unsigned|uint32_t|int)\s+flags,\s*int \*ok,\s*char \*\*\w+\)", code)
    from tkmk import service
    assert "tkmk_crs_audit_files_ex" in service.SYMBOLS
    for testing in (False, True):
        lib = service.lib(testing)
        for name in ("tkmk_crs_audit_files_ex", "tkmk_crs_audit_files", "tkmk_crs_audit_circuit_files"):
            assert hasattr(lib, name), name
        ok = ctypes.c_int(-1)                                       # a null directory is refused before anything is read
        lib.tkmk_crs_audit_files_ex.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
        assert lib.tkmk_crs_audit_files_ex(None, b"/nonexistent", 3, ctypes.byref(ok), None) != 0
        assert lib.tkmk_crs_audit_files_ex(b"/nonexistent", b"/nonexistent", 4, ctypes.byref(ok), None) != 0   # an unknown flag


def test_crs_check_usage_lists_locate():
    r = subprocess.run([CRS_CHECK, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--locate" in r.stdout and "--circuit" in r.stdout
    r = subprocess.run([CRS_CHECK, "--locate"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--crs" in r.stderr and "--locate" in r.stderr
    r = subprocess.run([CRS_CHECK, "--circuit", "--locate"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
