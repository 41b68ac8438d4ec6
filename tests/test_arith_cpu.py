"""WCPT_OPTION_ARITH on the host side (no GPU): wcpt_last_arith is exported and rejects a null handle, and the Python
mirror's ARITH_* values are the header's."""
import ctypes as C
import os
import re

import wcpt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wcpt.h")


def test_last_arith_exported():
    lib = C.CDLL(wcpt.LIB_PATH)
    assert hasattr(lib, "wcpt_last_arith")
    assert "wcpt_last_arith" in wcpt.EXPORTED_SYMBOLS


def test_last_arith_rejects_null_handle():
    v = C.c_int(-7)
    assert wcpt.lib.wcpt_last_arith(None, C.byref(v)) == wcpt._lib.WCPT_ERROR_INVALID_HANDLE
    assert v.value == -7


def test_arith_constants_match_header():
    text = open(HEADER).read()
    values = dict(re.findall(r"#define WCPT_ARITH_(\w+)\s+(\d+)", text))
    assert set(values) == {"EXACT", "FAST"}
    for name, value in values.items():
        assert getattr(wcpt._lib, "ARITH_" + name) == int(value), name
    assert wcpt._lib.ARITH_EXACT == 0 and wcpt._lib.ARITH_FAST == 1
    assert wcpt._lib.OPTION_ARITH == int(re.search(r"#define WCPT_OPTION_ARITH\s+(\d+)", text).group(1)) == 17
