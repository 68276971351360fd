"""lpg_batch's host-side validation and build wiring (no GPU: every check
here is answered before the library touches a device)."""
from __future__ import annotations

import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from linearprogramming_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("count,m,ncols,flags,word", [
    (0, 4, 9, 0, "count"),                 # count = 0
    (4, 0, 9, 0, "m"),                     # m = 0
    (4, 4, 1, 0, "ncols"),                 # ncols < 2
    (4, 4, 9, 0x4, "flags"),               # LPG_FLAG_BIG_M
    (4, 4, 9, 0x8, "flags"),               # LPG_FLAG_EAGER
    (4, 4, 9, 0x2, "flags"),               # LPG_FLAG_NO_SKIP
    (4, 4, 8193, 0, "lpg_create"),         # ncols > 8192: points to the single-LP engine
    (4, 8192, 9, 0, "lpg_create"),         # m + 1 > 8192
])
def test_create_refuses_bad_arguments_with_a_message(lib, count, m, ncols, flags, word):
    from linearprogramming_amd import _lib
    b = ctypes.c_void_p(1)
    rc = lib.lpg_batch_create(ctypes.byref(b), 0, count, m, ncols, flags)
    assert rc == _lib.ERR_ARG
    assert not b.value                                   # *out cleared
    msg = lib.lpg_batch_last_error(None).decode()
    assert msg and word in msg, msg


def test_python_wrapper_raises_with_the_message():
    import linearprogramming_amd as lpg
    with pytest.raises(lpg.LPGError, match="rc=-1.*bad shape"):
        lpg.BatchEngine(0, 4, 9)


def test_null_handles_are_errors_not_crashes(lib):
    from linearprogramming_amd import _lib
    lib.lpg_batch_destroy(None)
    assert lib.lpg_batch_solve(None, 10, 0, None) == _lib.ERR_ARG
    assert lib.lpg_batch_solve_dual(None, 10, None) == _lib.ERR_ARG
    assert lib.lpg_batch_info(None, None) == _lib.ERR_ARG
    assert lib.lpg_batch_get_log(None, 0, None, None, 0) == _lib.ERR_ARG


def test_every_source_list_names_the_batch_file():
    """The product objects and the two lab libraries (phases, pub) are built
    from explicit lists; a translation unit missing from one of them would
    leave that library without the lpg_batch_* symbols the header declares."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    kobjs = re.search(r"^KOBJS\s*=(.*)$", mk, flags=re.M).group(1)
    assert "$(OBJDIR)/lpg_batch.o" in kobjs
    for target in ("tools/probe/liblpg_phases.so", "tools/probe/liblpg_pub.so"):
        rule = re.search(r"^" + re.escape(target) + r":(.*)\n\t.*\n\t(.*)$", mk, flags=re.M)
        assert rule, target
        assert "$(CSRC)/lpg_batch.hip" in rule.group(1), target      # prerequisites
        assert "$(CSRC)/lpg_batch.hip" in rule.group(2), target      # the compile line
