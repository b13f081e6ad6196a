"""The ctypes binding is parsed from include/cosnet_hip.h (cosnet_amd/_native.py::signatures):
pinned prototypes read off the header, the entry-point count, and the closed type map.  No
library and no GPU needed.
"""
import ctypes
import os
import re

import pytest

from conftest import REPO
from cosnet_amd import _native

I, L, F, D, S, P = (ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double, ctypes.c_size_t,
                    ctypes.c_void_p)


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(REPO, "include", "cosnet_hip.h")) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def sigs(header):
    return _native.signatures(header)


def test_pinned_signatures(sigs):
    res, args, names = sigs["cn_gemm"]
    assert res is I and len(args) == 25 and len(names) == 25
    assert [n for n, t in zip(names, args) if t is F] == ["alpha"]
    assert args == [I] * 8 + [P, L, L, P, L, L, P, L, L, I, I, F, P, I, I, L, P]
    assert names[:3] == ["dtype", "layout_a", "layout_b"] and names[-2:] == ["slab", "stream"]

    res, args, names = sigs["cn_bce_l1_devcount"]
    assert args == [P, P, L, P, D, F, P, P, P, P] and names[4] == "total"
    assert [k for k, (_, a, _) in sigs.items() if D in a] == ["cn_bce_l1_devcount"]

    # `float* ws /* cn_avgpool_workspace_floats() */`: a comment inside the parameter list
    assert sigs["cn_avgpool"] == (I, [I, P, L, I, I, I, F, P, P, P],
                                  ["dtype", "x", "ld", "N", "HW", "C", "scale", "y", "ws", "stream"])
    assert sigs["cn_gemm_ws_launches"] == (S, [], [])                      # (void)
    assert sigs["cn_build_source_hash"] == (ctypes.c_char_p, [], [])
    # `float* const* dws`, `const float* const* x_states` and `const int* ia` are all pointers
    res, args, names = sigs["cn_conv_wgrad_fp8"]
    assert len(args) == 23
    assert [n for n, t in zip(names, args) if t is P] == ["xs8", "dys8", "dws", "x_states", "dy_states", "ws",
                                                          "stream"]
    assert not [t for t in args if t is F] and names[-3:] == ["ws", "ws_floats", "stream"]
    res, args, names = sigs["cn_coatt_fused_fwd_idx"]
    assert len(args) == 17
    assert [n for n, t in zip(names, args) if t is P] == ["vat", "va", "vb", "ia", "ib", "za", "zb", "ws", "stream"]
    assert names[-3:] == ["ws", "ws_bytes", "stream"]


def test_parse_finds_every_declared_entry_point(header, sigs):
    names = set(re.findall(r"^(?:int|size_t|const char\*)\s+(cn_\w+)\(", header, re.M))
    assert len(names) == 94
    assert set(sigs) == names == set(_native.exported_symbols())
    assert all(len(args) == len(pnames) for _, args, pnames in sigs.values())


def test_rejected_argument_is_named():
    """An argument ctypes refuses never reaches the library; the error names the C parameter."""
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    with pytest.raises(_native.NativeError, match=r"cn_bn_set_tuning: argument 2 \(value\)"):
        _native.call("cn_bn_set_tuning", 0, "not an int")


def test_unknown_type_raises_and_names_keep_their_order():
    ok = "int cn_x(int a, const float* b /* note, with a comma */, long long c,\n         hipStream_t stream);"
    assert _native.signatures(ok) == {"cn_x": (I, [I, P, L, P], ["a", "b", "c", "stream"])}
    for bad in ("int cn_x(short a, int b);", "int cn_x(int a, unsigned b);", "int cn_x(int);",
                "double cn_x(int a);", "void* cn_x(void);"):
        with pytest.raises(_native.NativeError):
            _native.signatures(bad)
