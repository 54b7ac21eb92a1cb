"""The development build's record of error returns taken, a site being (host unit, source line): rcw_dev_fail_unit(u) names host unit u
(NULL past the last), rcw_dev_fail_sites(u, out, cap) hands out the lines of that unit taken so far (csrc/rcw_error.h, rcw_api.hip).
Several units share line numbers, so a refusal must land in the unit that holds its `fail(`, and in no other:

  * a NULL handle is refused by check_handle                                    rcw_api.hip
  * a form asked of a configuration without a top view, by top_view_rule        rcw_rules.hip
  * a NULL unique id, by rcw_comm_unique_id in front of any load of RCCL        rcw_comm.hip

For each call exactly one new site appears, the line of that file at that number holds a `fail(`, and rcw_last_error() is the text
on that line.  No site of rcw_step.hip can be reached without a device: tests/failsite_plugin.py covers that unit in a run of the
GPU suite with the plugin loaded."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raycastworlds.jl_amd", "csrc")
UNITS = ["rcw_api.hip", "rcw_rules.hip", "rcw_step.hip", "rcw_comm.hip"]


@pytest.fixture(scope="module")
def devlib(rcw):
    from raycastworlds_jl_amd import _capi

    if not os.path.exists(_capi.DEV_LIB_PATH):
        from raycastworlds_jl_amd import build as _build

        _build.build()
    lib = _capi.load("dev")
    lib.rcw_dev_fail_unit.argtypes = [C.c_int]
    lib.rcw_dev_fail_unit.restype = C.c_char_p
    lib.rcw_dev_fail_sites.argtypes = [C.c_int, C.POINTER(C.c_ubyte), C.c_int]
    return lib


def _units(lib):
    names = []
    while (name := lib.rcw_dev_fail_unit(len(names))) is not None:
        names.append(name.decode())
    return names


def _sites(lib):
    taken = set()
    for u, name in enumerate(_units(lib)):
        buf = (C.c_ubyte * 4096)()
        n = lib.rcw_dev_fail_sites(u, buf, 4096)
        assert n == 4096
        taken |= {(name, i) for i in range(n) if buf[i]}
    return taken


def _null_handle(lib, _capi):
    return lib.rcw_sync(None)


def _form_without_a_top_view(lib, _capi):
    cfg = _capi.default_config()
    cfg.render_top_view = 0
    out = (C.c_int32 * 16)()
    lib.rcw_dev_plan_top_view.argtypes = [C.POINTER(_capi.RcwConfig), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    return lib.rcw_dev_plan_top_view(C.byref(cfg), 4, 256, 160 * 1024, 32, _capi.RCW_TOP_VIEW_ONE_KERNEL, 0, out)


def _null_unique_id(lib, _capi):
    return lib.rcw_comm_unique_id(None)


@pytest.mark.parametrize("call, unit, code, text", [
    (_null_handle, "rcw_api.hip", "RCW_ERR_INVALID_ARGUMENT", "NULL handle"),
    (_form_without_a_top_view, "rcw_rules.hip", "RCW_ERR_UNSUPPORTED", "handle was created with render_top_view = 0"),
    (_null_unique_id, "rcw_comm.hip", "RCW_ERR_INVALID_ARGUMENT", "NULL argument"),
], ids=["api", "rules", "comm"])
def test_a_refusal_is_recorded_in_the_unit_that_holds_it(devlib, call, unit, code, text):
    from raycastworlds_jl_amd import _capi

    before = _sites(devlib)
    rc = call(devlib, _capi)
    new = _sites(devlib) - before
    assert rc == getattr(_capi, code)
    assert len(new) == 1, new
    (name, line), = new
    assert name == unit
    source = open(os.path.join(CSRC, name)).read().splitlines()[line - 1]
    assert "fail(" in source, (name, line, source)
    message = re.search(r'fail\(\w+, "((?:[^"\\]|\\.)*)"', source).group(1)
    assert message == text and _capi.last_error(devlib) == message


def test_the_units_are_the_four_host_units_and_nothing_lies_past_the_last(devlib):
    assert _units(devlib) == UNITS
    for name in UNITS:
        assert os.path.exists(os.path.join(CSRC, name))
    buf = (C.c_ubyte * 4096)()
    for u in (-1, len(UNITS), len(UNITS) + 1, 1 << 20):
        assert devlib.rcw_dev_fail_unit(u) is None
        assert devlib.rcw_dev_fail_sites(u, buf, 4096) == -1
    assert not any(buf)
    assert devlib.rcw_dev_fail_sites(0, None, 4096) == -1 and devlib.rcw_dev_fail_sites(0, buf, 0) == -1
