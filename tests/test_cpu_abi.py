"""CPU: the Python side of the C ABI is read from include/aptai_hip.h (aptai_amd/_abi.py), never typed a second time.  Checked against
the host C compiler (struct layouts), against an independent count of every prototype's parameters, against literal pins of the
places a type-mapping bug would hide, and for strictness: what the reader does not know raises and names the symbol."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from aptai_amd import _abi, _lib, ops

STRUCTS = {"aptai_gemm_desc": ops.GemmDesc, "aptai_gemm_plan_info": ops.GemmPlanInfo}


def _header_without_comments() -> str:
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "aptai_hip.h")).read(), flags=re.S)


def test_struct_layouts_match_the_c_compiler(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "aptai_hip.h"', 'int main(void) {']
    for cname, cls in STRUCTS.items():
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    py = {}
    for cname, cls in STRUCTS.items():
        py[cname] = str(ctypes.sizeof(cls))
        py.update({f"{cname}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert py == c
    assert (py["aptai_gemm_desc"], py["aptai_gemm_plan_info"]) == ("320", "32")
    assert (py["aptai_gemm_desc.tile"], py["aptai_gemm_desc.split_out_bcol"]) == ("280", "316")
    assert len(ops.GemmDesc._fields_) == 41 and len(ops.GemmPlanInfo._fields_) == 6


def test_every_declared_symbol_carries_its_prototype():
    text = _header_without_comments()
    protos = {m.group(2): (m.group(1), m.group(3).strip())
              for m in re.finditer(r"\b(int64_t|int|const char\*)\s+(aptai_\w+)\s*\(([^()]*)\)\s*;", text)}
    names = _lib.declared_symbols()
    assert sorted(protos) == names and len(names) >= 109
    L = _lib.lib()
    for n in names:
        ret, params = protos[n]
        assert len(_lib.ARGTYPES[n]) == (0 if params == "void" else params.count(",") + 1), n
        fn = getattr(L, n)
        assert fn.argtypes == _lib.ARGTYPES[n], n
        assert fn.restype is {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "const char*": ctypes.c_char_p}[ret], n
    assert [n for n in names if protos[n][0] == "const char*"] == ["aptai_last_error"]
    assert all(n.endswith("_workspace_bytes") for n in names if protos[n][0] == "int64_t")


def test_literal_pins_of_the_type_mapping():
    P, I64, I, F, U64 = _lib._P, _lib._I64, _lib._I, _lib._F, _lib._U64
    assert (P, I64, I, F, U64) == (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint64)
    A = _lib.ARGTYPES
    assert A["aptai_grad_sqnorm_multi"][6] is ctypes.c_double
    assert A["aptai_eval_boundary_counts"][6] is ctypes.c_double
    assert A["aptai_device_check"] == [ctypes.c_char_p, I]
    assert A["aptai_gemm_bf16"] == [P, P] and A["aptai_gemm_bf16_grouped"] == [P, I, P]
    assert A["aptai_gemm_bf16_grouped_rowsum"] == [P, P, I, P]
    assert A["aptai_dropout_bf16"] == [P, P, I64, F, U64, P]
    assert A["aptai_version"] == [] and A["aptai_last_error"] == []
    assert ops.EPI_SPLIT_OUT == 512 and ops.EPI_BIAS_ROW == 1024        # listed out of numeric order in the header
    assert [ops.EPI_BIAS, ops.EPI_GELU, ops.EPI_RESIDUAL, ops.EPI_DROPOUT, ops.EPI_DGELU, ops.EPI_ALPHA, ops.EPI_PRE_DGELU,
            ops.EPI_MUL_AUX, ops.EPI_RESIDUAL_F32] == [1 << i for i in range(9)]
    assert ops.RESAMPLE_MAX_TABLE == 1 << 22 and ops.RESAMPLE_MAX_RATIOS == 8 and ops.EVAL_EDIT_MAX_LANE_SIDE == 2048
    assert _abi.header() is _abi.header() is _lib.ABI                   # one parse per process


def test_the_reader_parses_the_forms_the_header_uses():
    abi = _abi.parse("""
        /* a comment with int aptai_not_a_function(int x); inside */
        #ifndef G
        #define G
        #define APTAI_N (1 << 4)
        enum { APTAI_A = 1, APTAI_C = 0x10, APTAI_B = -2 };
        typedef struct { const void* p; int64_t m, n; float* const* q;
                         uint64_t s[2],
                             t[3]; double d; } thing;
        const char* aptai_text(void);
        int64_t aptai_bytes(const thing* t, char* name, const char* src, float* const* rows, uint64_t seed, double tol,
                            float eps, int n);
        #endif
    """)
    assert abi.constants == {"APTAI_N": 16, "APTAI_A": 1, "APTAI_C": 16, "APTAI_B": -2}
    assert abi.structs["thing"] == [("p", ctypes.c_void_p), ("m", ctypes.c_int64), ("n", ctypes.c_int64), ("q", ctypes.c_void_p),
                                    ("s", ctypes.c_uint64 * 2), ("t", ctypes.c_uint64 * 3), ("d", ctypes.c_double)]
    assert abi.prototypes == {"aptai_text": (ctypes.c_char_p, []),
                              "aptai_bytes": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p,
                                                               ctypes.c_uint64, ctypes.c_double, ctypes.c_float, ctypes.c_int])}


@pytest.mark.parametrize("text, names", [
    ("int aptai_takes_size(const float* x, size_t count, void* stream);", ("aptai_takes_size", "count", "size_t")),
    ("int aptai_ptr_to_unknown(const size_t* sizes);", ("aptai_ptr_to_unknown", "sizes", "size_t")),
    ("size_t aptai_returns_size(void);", ("aptai_returns_size", "size_t")),
    ("int aptai_by_value(aptai_rec0 whole);", ("aptai_by_value", "whole", "aptai_rec0")),
    ("int aptai_no_parameters();", ("aptai_no_parameters",)),
    ("typedef struct { int64_t rows; size_t pitch; } aptai_rec;", ("aptai_rec", "pitch", "size_t")),
    ("typedef struct { int* first, second; } aptai_rec;", ("aptai_rec", "first")),
    ("typedef struct { int (*callback)(int); } aptai_rec;", ("callback",)),
    ("#define APTAI_X 1.5f", ("APTAI_X", "1.5f")),
    ("#define APTAI_X sizeof(int)", ("APTAI_X",)),
    ("enum { APTAI_FIRST, APTAI_SECOND = 2 };", ("APTAI_FIRST",)),
    ("int aptai_fine(int n);\nstatic inline int aptai_helper(int n) { return n; }", ("aptai_helper",)),
])
def test_the_reader_refuses_what_it_does_not_know(text, names):
    with pytest.raises(_abi.AbiError) as e:
        _abi.parse("typedef struct { int v; } aptai_rec0;\n" + text)
    for n in names:
        assert n in str(e.value), (n, str(e.value))
