"""CPU: the surface of drx_transcode's block form -- the two queries, the DRX_TRANSCODE_FORM_* values and the two debug flags,
equal in the header, the built library and the Python binding; every debug flag one bit and none twice; a NULL plan."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()


def test_queries_forms_and_flags_agree():
    from deltarice_amd import _lib, codec
    lib = _lib.load()
    txt = _header()
    for name in ("drx_plan_last_transcode_form", "drx_plan_last_transcode_listed"):
        assert re.search(r"^uint32_t " + name + r"\(const drx_plan \*plan\);", txt, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_uint32 and args == [_lib.C.c_void_p], name
    defs = {k: int(v) for k, v in re.findall(r"^#define DRX_(\w+) (\d+)u\b", txt, flags=re.M)}
    assert (defs["TRANSCODE_FORM_LANES"], defs["TRANSCODE_FORM_BLOCKS"], defs["TRANSCODE_FORM_FALLBACK_ALL"]) == (1, 2, 4)
    assert (_lib.TRANSCODE_FORM_LANES, _lib.TRANSCODE_FORM_BLOCKS, _lib.TRANSCODE_FORM_FALLBACK_ALL) == (1, 2, 4)
    assert defs["DBG_TRANSCODE_LANES"] == 1024 == _lib.DBG_TRANSCODE_LANES
    assert defs["DBG_TRANSCODE_ALL_FALLBACK"] == 16384 == _lib.DBG_TRANSCODE_ALL_FALLBACK
    assert callable(codec.Plan.last_transcode_form) and callable(codec.Plan.last_transcode_listed)


def test_every_debug_flag_is_one_bit_and_none_twice():
    from deltarice_amd import _lib
    defs = {k: int(v) for k, v in re.findall(r"^#define DRX_(DBG_\w+) (\d+)u\b", _header(), flags=re.M)}
    values = list(defs.values())
    assert all(v and v & (v - 1) == 0 and v < (1 << 32) for v in values), defs
    assert len(set(values)) == len(values), defs
    # ... and the binding has every one of them, with the header's value
    bound = {k: v for k, v in vars(_lib).items() if k.startswith("DBG_")}
    assert bound == defs, (sorted(set(bound.items()) ^ set(defs.items())))


def test_a_null_plan_has_no_form():
    from deltarice_amd import _lib
    lib = _lib.load()
    assert lib.drx_plan_last_transcode_form(None) == 0
    assert lib.drx_plan_last_transcode_listed(None) == 0
