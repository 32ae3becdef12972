"""yl_create's validation runs on the host, before any device call: every case of tests/_create_cases.py gives the status
and the message recorded in tests/golden/create_errors.json (tests/golden/make_create_fixtures.py: recorded behind a
device, with the library of the commit before the validation moved into csrc/yl_program.cpp) -- on a machine with a HIP
device and on one without.  Not a gpu test: it launches nothing."""
import ctypes
import json
import os
import re

import pytest

from _create_cases import BASES, CASES, MESSAGE_TEXTS, build_case, create
from yololite_amd import _lib

YL_ERR_HIP = -2       # include/yololite_hip.h

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_errors.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _device_count():
    """devices the HIP runtime the library links against can use (0 on a CPU-only machine)"""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        return 0
    n = ctypes.c_int(0)
    return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else 0


def test_cases_cover_every_message_text():
    assert sorted(RECORDED["cases"]) == sorted(name for name, _, _ in CASES)
    texts = {re.sub(r"^layer \d+: ", "", msg) for _, msg in RECORDED["cases"].values()}
    assert len(texts) >= MESSAGE_TEXTS
    assert all(st != _lib.YL_OK and msg for st, msg in RECORDED["cases"].values())


@pytest.mark.parametrize("name,base,edit", CASES, ids=[c[0] for c in CASES])
def test_invalid_description_reports_the_recorded_error(lib, name, base, edit):
    d, keep = build_case(base, edit)
    st, msg, h = create(lib, d)
    assert h, "the context is handed out for yl_last_error"
    lib.yl_destroy(h)
    assert [st, msg] == RECORDED["cases"][name]


def test_two_faulty_layers_report_the_first(lib):
    assert RECORDED["cases"]["two_faulty_layers"][1].startswith("layer 2: ")


@pytest.mark.parametrize("base", list(BASES))
def test_valid_description_needs_a_device(lib, base):
    d, keep = build_case(base)
    st, msg, h = create(lib, d)
    if _device_count() > 0:
        assert st == RECORDED["valid"][base] == _lib.YL_OK and h
        lib.yl_destroy(h)
    else:
        assert st == YL_ERR_HIP and not h
