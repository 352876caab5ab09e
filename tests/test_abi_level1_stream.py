"""CPU tests of the Level1 cursor's C ABI (include/mcs.h, include/mcs_trade.h): the four entry points are
declared, exported and bound, the stats struct has its C layout, and a null handle is refused."""
import ctypes as C
import os
import re
import subprocess

import mcs_amd
from mcs_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mcs_stream_open_level1", "mcs_stream_next_level1", "mcs_trade_stream_open_level1",
         "mcs_trade_stream_next_level1"]


def test_the_four_symbols_are_declared_exported_and_bound():
    lib = mcs_amd.lib()
    text = "".join(open(os.path.join(REPO, "include", h)).read() for h in ("mcs.h", "mcs_trade.h"))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (mcs_[a-z0-9_]+)$", out.stdout, flags=re.M))
    bound = {name: args for name, _, args in L.SIGNATURES}
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in exported and name in bound and hasattr(lib, name), name
    assert len(bound["mcs_stream_next_level1"]) == len(bound["mcs_stream_next"]) + 2
    assert len(bound["mcs_trade_stream_next_level1"]) == len(bound["mcs_trade_stream_next"]) + 2
    assert lib.mcs_abi_version() == 7  # additive: the version stays


def test_stats_struct_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcs_trade.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu\\n", sizeof(mcs_level1_stream_stats), '
                   'offsetof(mcs_level1_stream_stats, rows_scanned), offsetof(mcs_level1_stream_stats, kernel_ms));\n'
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    size, o_rows, o_ms = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert (size, o_rows, o_ms) == (16, 0, 8)
    assert C.sizeof(L.mcs_level1_stream_stats) == 16
    assert L.mcs_level1_stream_stats.rows_scanned.offset == 0 and L.mcs_level1_stream_stats.kernel_ms.offset == 8


def test_a_null_handle_is_refused():
    lib = mcs_amd.lib()
    assert lib.mcs_stream_open_level1(None, 0, 5, 0) == L.MCS_E_INVALID
    assert lib.mcs_trade_stream_open_level1(None, 0, 5, 0) == L.MCS_E_INVALID
    assert lib.mcs_stream_next_level1(None, 4, None, None, None, 0, None, None) == L.MCS_E_INVALID
    assert lib.mcs_trade_stream_next_level1(None, 4, None, None, None, 0, None, None) == L.MCS_E_INVALID
