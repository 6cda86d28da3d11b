"""CPU: the surface of drx_find_pulses' block form -- the query that says which form ran, its values, the two debug flags --
in the header, the built library and deltarice_amd/_lib.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_python_agree():
    from deltarice_amd import _lib, codec
    txt = open(os.path.join(ROOT, "include", "deltarice_hip.h")).read()
    assert re.search(r"^uint32_t drx_plan_last_pulses_form\(const drx_plan \*plan\);", txt, flags=re.M)
    forms = {k: int(v) for k, v in re.findall(r"^#define DRX_(PULSES_FORM_\w+) (\d+)u\b", txt, flags=re.M)}
    assert forms == {"PULSES_FORM_LANES": 1, "PULSES_FORM_BLOCKS": 2, "PULSES_FORM_FALLBACK_ALL": 4}, forms
    flags = {k: int(v) for k, v in re.findall(r"^#define DRX_(DBG_\w+) (\d+)u\b", txt, flags=re.M)}
    mine = {"DBG_PULSES_LANES": flags["DBG_PULSES_LANES"], "DBG_PULSES_ALL_FALLBACK": flags["DBG_PULSES_ALL_FALLBACK"]}
    # one bit each, none twice, both above DRX_DBG_STATS_ALL_FALLBACK and inside the 32-bit option word
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values())
    assert all(flags["DBG_STATS_ALL_FALLBACK"] < v < 1 << 32 for v in mine.values()), mine
    for name, value in {**forms, **mine}.items():
        assert getattr(_lib, name) == value, name
    lib = _lib.load()
    assert hasattr(lib, "drx_plan_last_pulses_form") and "drx_plan_last_pulses_form" in _lib.SIGNATURES
    assert lib.drx_plan_last_pulses_form(None) == 0  # (no plan: nothing ran)
    assert callable(codec.Plan.last_pulses_form)
    assert re.search(r"^uint32_t drx_plan_last_pulses_listed\(const drx_plan \*plan\);", txt, flags=re.M)
    assert hasattr(lib, "drx_plan_last_pulses_listed") and lib.drx_plan_last_pulses_listed(None) == 0
    assert callable(codec.Plan.last_pulses_listed)
    assert re.search(r"^uint32_t drx_plan_last_pulses_redone\(const drx_plan \*plan\);", txt, flags=re.M)
    assert hasattr(lib, "drx_plan_last_pulses_redone") and lib.drx_plan_last_pulses_redone(None) == 0
    assert callable(codec.Plan.last_pulses_redone)
    cap = re.search(r"^#define DRX_PULSES_STAGE_CAP (\d+)u\b", txt, flags=re.M)
    assert cap and int(cap.group(1)) == _lib.PULSES_STAGE_CAP
    src = open(os.path.join(ROOT, "deltarice_amd", "csrc", "drx_pulses_blocks.hip")).read()
    assert "kPulseStageCap = DRX_PULSES_STAGE_CAP;" in src  # (the kernel file takes the header's)
