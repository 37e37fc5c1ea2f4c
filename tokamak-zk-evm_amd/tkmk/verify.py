"""ctypes binding of the verifier's entries of libtkmk_prover.so (include/tkmk_prover.h; host/tkmk_verify.hpp over host/tkmk_pairing.hpp):
the work-alike of the reference's `verify` (packages/backend/verify-rust/src/lib.rs: Verifier::init + verify_snark) as library calls.
Host-only — none of them touches a device, except the batch entries on route="device", which the caller asks for; the same code is the binary tokamak-zk-evm_amd/bin/verify.  Nothing here is Python
beyond the call itself."""
import ctypes
import json
import os

import numpy as np

from tkmk import service


def _lib(testing=False):
    l = service.lib(testing)
    if not getattr(l, "_tkmk_verify_bound", False):
        l.tkmk_pairing_product_is_one.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        l.tkmk_verify_files.argtypes = [ctypes.c_char_p] * 5 + [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]
        l.tkmk_prover_verify.argtypes = [ctypes.c_void_p] + [ctypes.c_char_p] * 3 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]
        l.tkmk_crs_audit_files.argtypes = [ctypes.c_char_p] * 2 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]
        l.tkmk_crs_audit_circuit_files.argtypes = l.tkmk_crs_audit_files.argtypes
        l.tkmk_crs_audit_files_ex.argtypes = [ctypes.c_char_p] * 2 + [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]
        l.tkmk_witness_check_files.argtypes = [ctypes.c_char_p] * 2 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]
        l.tkmk_prover_check_witness.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]
        l.tkmk_prover_check_witness_sharded.argtypes = l.tkmk_prover_check_witness.argtypes
        tail = [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]
        l.tkmk_verify_batch_files.argtypes = [ctypes.c_char_p] * 2 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32] + tail
        l.tkmk_prover_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + tail
        l._tkmk_verify_bound = True
    return l


ROUTE_HOST, ROUTE_DEVICE = 0, 1            # TKMK_VERIFY_ROUTE_* of include/tkmk_prover.h


class VerifyItem(ctypes.Structure):        # tkmk_verify_item
    _fields_ = [("synthesizer_dir", ctypes.c_char_p), ("preprocess_dir", ctypes.c_char_p), ("proof_dir", ctypes.c_char_p)]


def _items(items):
    arr = (VerifyItem * max(len(items), 1))()
    for k, (synth, pre, proof) in enumerate(items):
        arr[k] = VerifyItem(os.fsencode(synth), os.fsencode(pre), os.fsencode(proof))
    return arr


def _route(route):
    return {"host": ROUTE_HOST, "device": ROUTE_DEVICE}.get(route, route)


def _g1_record(p):
    if p is None:
        return bytes(96)
    b = bytes(np.asarray(p, np.uint8))
    if len(b) != 96:
        raise ValueError("a G1 point is a 96-byte affine record (x, y little-endian; all zero = infinity)")
    return b


def _g2_record(q):
    from tkmk import g2
    if q is None:
        return bytes(192)
    if isinstance(q, tuple):
        (x0, x1), (y0, y1) = q                 # tkmk.g2 representation; values are NOT reduced here: the library checks the range
        return b"".join(int(v).to_bytes(48, "little") for v in (x0, x1, y0, y1))
    b = bytes(np.asarray(q, np.uint8))
    if len(b) != 192:
        raise ValueError("a G2 point is a tkmk.g2 point or its 192-byte record")
    return b


def pairing_product_is_one(pairs, testing=False):
    """pairs: [(P, Q)], P a 96-byte G1 affine record or None, Q a tkmk.g2 point, its 192-byte record or None (None = infinity).
    -> True iff prod e(P, Q) = 1.  service.ProverError (TKMK_ERR_INVALID_ARGUMENT, the message names index and reason) for a point
    off its curve, outside the subgroup of order r, or with a coordinate >= p."""
    l = _lib(testing)
    g1 = b"".join(_g1_record(p) for p, _ in pairs)
    g2 = b"".join(_g2_record(q) for _, q in pairs)
    out = ctypes.c_int(-1)
    code = l.tkmk_pairing_product_is_one(ctypes.c_char_p(g1) if pairs else None, ctypes.c_char_p(g2) if pairs else None, len(pairs), ctypes.byref(out))
    if code != 0:
        raise service.ProverError(code, "tkmk_pairing_product_is_one", testing)
    return out.value == 1


def _take_report(l, doc):
    rep = json.loads(ctypes.string_at(doc.value).decode())
    l.tkmk_prover_free_string(doc)
    return rep


def verify_files(subcircuit_library_dir, crs_dir, synthesizer_dir, preprocess_dir, proof_dir, root_generator=0, testing=False):
    """-> (ok, report): the decision of the reference's `verify` over the same five directories, and the report
    {"generator", "ok", "reason", "thetas", "kappa0", "chi", "zeta", "kappa1", "a_eval"} (scalars as hex strings).
    root_generator = 0: TKMK_FR_ROOT_GENERATOR, else the declared default.  service.ProverError for unreadable input."""
    l = _lib(testing)
    ok, doc = ctypes.c_int(-1), ctypes.c_void_p()
    code = l.tkmk_verify_files(os.fsencode(subcircuit_library_dir), os.fsencode(crs_dir), os.fsencode(synthesizer_dir), os.fsencode(preprocess_dir),
                               os.fsencode(proof_dir), int(root_generator), ctypes.byref(ok), ctypes.byref(doc))
    if code != 0:
        raise service.ProverError(code, "tkmk_verify_files", testing)
    return ok.value == 1, _take_report(l, doc)


def verify_batch(subcircuit_library_dir, crs_dir, items, root_generator=0, route="host", testing=False):
    """tkmk_verify_batch_files: items = [(synthesizer_dir, preprocess_dir, proof_dir)], proofs of ONE circuit against ONE reference string
    -> (ok_each: list of bool, report).  ok_each[k] is what verify_files says for item k alone; an all-honest batch costs one product of
    ten pairings (report["products"] == 1), false items are isolated by bisection with fresh weights.  route: "host" (no device call) or
    "device" (one tkmk_g1_check, per fold one tkmk_msm_segmented call and, for slot jobs too long for it, one tkmk_msm_multi_ex call;
    TKMK_ERR_NO_DEVICE without one).  report = {"generator", "ok", "n", "route", "products", "segmented_jobs", "pipeline_jobs" (the device
    route's slot jobs by MSM entry, over all folds), "items": [a verify_files report per item], "seconds"}.  service.ProverError for an empty batch (code 11) and for
    unreadable input (the message names the item and the file)."""
    l = _lib(testing)
    each, ok, doc = (ctypes.c_uint8 * max(len(items), 1))(), ctypes.c_int(-1), ctypes.c_void_p()
    code = l.tkmk_verify_batch_files(os.fsencode(subcircuit_library_dir), os.fsencode(crs_dir), ctypes.cast(_items(items), ctypes.c_void_p), len(items),
                                     int(root_generator), _route(route), ctypes.cast(each, ctypes.c_void_p), ctypes.byref(ok), ctypes.byref(doc))
    if code != 0:
        raise service.ProverError(code, "tkmk_verify_batch_files", testing)
    rep = _take_report(l, doc)
    return [bool(v) for v in each[:len(items)]], rep


def verify_batch_with(prover, items, route="host"):
    """tkmk_prover_verify_batch: the same against the reference string and generator of an open service.Prover.  route="device" on a
    sharded context is refused (code 11): its ranks keep the host route"""
    l = _lib(prover.testing)
    each, ok, doc = (ctypes.c_uint8 * max(len(items), 1))(), ctypes.c_int(-1), ctypes.c_void_p()
    code = l.tkmk_prover_verify_batch(prover._h, ctypes.cast(_items(items), ctypes.c_void_p), len(items), _route(route), ctypes.cast(each, ctypes.c_void_p),
                                      ctypes.byref(ok), ctypes.byref(doc))
    if code != 0:
        raise service.ProverError(code, "tkmk_prover_verify_batch", prover.testing)
    rep = _take_report(l, doc)
    return [bool(v) for v in each[:len(items)]], rep


AUDIT_CIRCUIT, AUDIT_LOCATE = 1, 2         # TKMK_CRS_AUDIT_* of include/tkmk_prover.h


def crs_audit(subcircuit_library_dir, crs_dir, testing=False, circuit=False, locate=False):
    """-> (ok, report): tkmk_crs_audit_files — is the reference string <crs_dir>/combined_sigma.{tkcrs, rkyv} well formed for the circuit of
    <subcircuit_library_dir>: membership of every G1 record on the device (tkmk_g1_check) and of the ten G2 points on the host, the anchors,
    and the power structure of xy_powers by four MSMs and two pairing products.  report = {"ok", "reason", "sections": [{"name", "points",
    "infinity", "noncanonical", "off_curve", "not_in_subgroup", "first_bad"}], "g2", "anchors", "ratio_y", "ratio_x", "seconds"}.  Needs a
    device; service.ProverError for unreadable input.  testing=True: libtkmk_prover_testing.so, which honours TKMK_CRS_AUDIT_SEED.
    circuit=True: tkmk_crs_audit_circuit_files — after all of that, the gamma / eta / delta tables, the small delta tables and the single
    points against the circuit (<lib>/subcircuitInfo.json, <lib>/r1cs/) and sigma_2; the report's "circuit" is then the verdict of those
    checks, "tables" = [{"name", "points", "ok"}] for gamma, eta, delta, delta_small, alpha_chain, singles and "table_seconds" their
    times (all three are None without it).
    locate=True: tkmk_crs_audit_files_ex with TKMK_CRS_AUDIT_LOCATE — a structural check that fails goes on to name the record: the
    report's "located" is then a list, in check order, of {"check", "section", "index", "row", "col", "more", "what"} (index None where the
    failure is not one record's, e.g. a wrong sigma_2.y; [] when nothing was located), "locate_products" the pairing products that took
    and "locate_seconds" their time; "reason" has the first finding's "what" appended.  Without circuit=True it covers xy_powers only.
    Without locate the call, its launches and its report text are what they were ("located" is None)."""
    l = _lib(testing)
    ok, doc = ctypes.c_int(-1), ctypes.c_void_p()
    if locate:
        name = "tkmk_crs_audit_files_ex"
        code = l.tkmk_crs_audit_files_ex(os.fsencode(subcircuit_library_dir), os.fsencode(crs_dir), AUDIT_LOCATE | (AUDIT_CIRCUIT if circuit else 0),
                                         ctypes.byref(ok), ctypes.byref(doc))
    else:
        name = "tkmk_crs_audit_circuit_files" if circuit else "tkmk_crs_audit_files"
        code = getattr(l, name)(os.fsencode(subcircuit_library_dir), os.fsencode(crs_dir), ctypes.byref(ok), ctypes.byref(doc))
    if code != 0:
        raise service.ProverError(code, name, testing)
    return ok.value == 1, _take_report(l, doc)


def witness_check(subcircuit_library_dir, synthesizer_dir, prover=None, testing=False, collective=False):
    """-> (ok, report): does the witness of <synthesizer_dir> (placementVariables.json, permutation.json, instance.json) satisfy the circuit
    of <subcircuit_library_dir>, and if not, where?  tkmk_witness_check_files: a device, no reference string.  prover = an open
    service.Prover: tkmk_prover_check_witness against that context's library (subcircuit_library_dir is then not read; a sharded context
    refuses with code 11).  collective=True (with prover): tkmk_prover_check_witness_sharded — EVERY rank of a sharded prover makes this
    call with the same arguments (dist.run_ranks over the loopback transport) and gets the same verdict and report; on an unsharded
    context it is the plain entry.  report = {"ok", "reason", "arithmetic": {"ok", "placements", "bad_placements", "bad_cells", "first"}, "copy":
    {"ok", "entries", "bijection", "bad_entries", "first"}, "public": {"ok", "wires", "bad", "first"}, "seconds"}: all three sections are
    always evaluated, `first` holds at most 8 findings each.  ok is what the verifier says about the proof made from the same documents.
    service.ProverError for an unreadable document (the message names the file) and without a device (code 12)."""
    l = _lib(prover.testing if prover is not None else testing)
    ok, doc = ctypes.c_int(-1), ctypes.c_void_p()
    if prover is not None:
        name, testing = "tkmk_prover_check_witness_sharded" if collective else "tkmk_prover_check_witness", prover.testing
        code = getattr(l, name)(prover._h, os.fsencode(synthesizer_dir), ctypes.byref(ok), ctypes.byref(doc))
    elif collective:
        raise ValueError("collective=True needs the prover whose ranks make the call")
    else:
        name = "tkmk_witness_check_files"
        code = l.tkmk_witness_check_files(os.fsencode(subcircuit_library_dir), os.fsencode(synthesizer_dir), ctypes.byref(ok), ctypes.byref(doc))
    if code != 0:
        raise service.ProverError(code, name, testing)
    return ok.value == 1, _take_report(l, doc)


def prover_verify(prover, synthesizer_dir, preprocess_dir, proof_dir):
    """the self-check of an open service.Prover: the same decision against the context's own reference string and root-of-unity
    generator -> (ok, report)"""
    l = _lib(prover.testing)
    ok, doc = ctypes.c_int(-1), ctypes.c_void_p()
    code = l.tkmk_prover_verify(prover._h, os.fsencode(synthesizer_dir), os.fsencode(preprocess_dir), os.fsencode(proof_dir), ctypes.byref(ok), ctypes.byref(doc))
    if code != 0:
        raise service.ProverError(code, "tkmk_prover_verify", prover.testing)
    return ok.value == 1, _take_report(l, doc)
