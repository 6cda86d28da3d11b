"""CPU: the surface of drx_wave_stats' block form -- the query that says which form ran, its values, the two debug flags --
in the header, the built library and deltarice_amd/_lib.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_python_agree():
    from deltarice_amd import _lib, codec
    txt = open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()
    assert re.search(r"^uint32_t drx_plan_last_stats_form\(const drx_plan \*plan\);", txt, flags=re.M)
    forms = {k: int(v) for k, v in re.findall(r"^#define DRX_(STATS_FORM_\w+) (\d+)u\b", txt, flags=re.M)}
    assert forms == {"STATS_FORM_LANES": 1, "STATS_FORM_BLOCKS": 2, "STATS_FORM_FALLBACK_ALL": 4}, forms
    flags = {k: int(v) for k, v in re.findall(r"^#define DRX_(DBG_\w+) (\d+)u\b", txt, flags=re.M)}
    assert flags["DBG_STATS_LANES"] == 67108864 and flags["DBG_STATS_ALL_FALLBACK"] == 134217728
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values())  # one bit each, none twice
    for name, value in {**forms, "DBG_STATS_LANES": flags["DBG_STATS_LANES"], "DBG_STATS_ALL_FALLBACK": flags["DBG_STATS_ALL_FALLBACK"]}.items():
        assert getattr(_lib, name) == value, name
    lib = _lib.load()
    assert hasattr(lib, "drx_plan_last_stats_form") and "drx_plan_last_stats_form" in _lib.SIGNATURES
    assert lib.drx_plan_last_stats_form(None) == 0  # (no plan: nothing ran)
    assert callable(codec.Plan.last_stats_form)
