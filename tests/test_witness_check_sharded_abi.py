"""not-gpu tier: the sharded witness check's two new symbols (tkmk_witness_check_copy_split, tkmk_prover_check_witness_sharded) resolve,
header and Python binding agree on their argument lists, and the collective entry takes the arguments of the entry it stands beside."""
from test_witness_check_abi import _ctype, _prototype


def test_symbols_resolve(tkmk):
    from tkmk import service
    assert "tkmk_witness_check_copy_split" in tkmk.SYMBOLS and hasattr(tkmk.lib(), "tkmk_witness_check_copy_split")
    for testing in (False, True):
        assert "tkmk_prover_check_witness_sharded" in service.SYMBOLS and hasattr(service.lib(testing), "tkmk_prover_check_witness_sharded")


def test_header_and_binding_agree_on_the_argument_lists(tkmk):
    from tkmk import verify
    declared = _prototype("tkmk.h", "tkmk_witness_check_copy_split")
    assert [_ctype(c) for c in declared] == tkmk.WITNESS_CHECK_ARGTYPES["tkmk_witness_check_copy_split"], declared
    assert declared == ["const tkmk_fr*", "uint64_t", "const uint32_t*", "const tkmk_fr*", "uint64_t", "const uint32_t*", "uint64_t", "uint64_t*", "uint64_t*",
                        "tkmk_stream"]
    assert _prototype("tkmk_prover.h", "tkmk_prover_check_witness_sharded") == _prototype("tkmk_prover.h", "tkmk_prover_check_witness")
    l = verify._lib()
    assert list(l.tkmk_prover_check_witness_sharded.argtypes) == list(l.tkmk_prover_check_witness.argtypes)


def test_null_results_are_refused_before_any_device_call(tkmk):
    import ctypes
    fn = tkmk._witness_check_fn("tkmk_witness_check_copy_split")
    bad = ctypes.c_uint64(7)
    assert fn(None, 0, None, None, 0, None, 0, None, None, None) == 3           # TKMK_ERR_INVALID_POINTER
    assert fn(None, 0, None, None, 0, None, 0, ctypes.byref(bad), None, None) == 3
