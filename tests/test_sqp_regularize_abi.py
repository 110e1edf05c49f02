"""CPU: the regularised-retry additions of the C ABI (ABI 13, additive: vc_set_sqp_regularization /
vc_get_sqp_regularization / vc_debug_sqp_breakdown) are declared by include/vcmpc.h, mirrored by
vcmpc._abi and exported by the library; no compute calls."""
import ctypes
import os
import re

from conftest import ROOT


def _header():
    src = open(os.path.join(ROOT, "include", "vcmpc.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_regularization_entry_points_and_keeps_abi_13():
    src = _header()
    assert re.search(r"\bint\s+vc_set_sqp_regularization\s*\(\s*vc_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*double\s+\w+\s*\)", src)
    assert re.search(r"\bint\s+vc_get_sqp_regularization\s*\(\s*vc_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", src)
    assert re.search(r"\bint\s+vc_debug_sqp_breakdown\s*\(\s*vc_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*int\s+\w+\s*\)", src)
    assert re.search(r"#define\s+VCMPC_ABI_VERSION\s+13\b", src)
    enum = re.search(r"enum\s+vc_status\s*\{(.*?)\}", src, flags=re.S).group(1)
    assert len(re.findall(r"VC_[A-Z_]+\s*=\s*\d+", enum)) == 5  # no new status value


def test_header_documents_diag_bits_64_and_128():
    src = open(os.path.join(ROOT, "include", "vcmpc.h")).read()
    doc = src[src.index("vc_solve plus per-problem solver diagnostics"):src.index("int vc_solve_diag(")]
    assert re.search(r"\b64 some QP broke down at every level", doc)
    assert re.search(r"\b128 some QP's applied step came from a level above 0", doc)


def test_abi_mirror_has_regularization_prototypes():
    from vcmpc import _abi
    assert _abi.ABI_VERSION == 13
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _abi.PROTOTYPES["vc_set_sqp_regularization"] == (i, [vp, i, ctypes.c_double])
    assert _abi.PROTOTYPES["vc_get_sqp_regularization"] == (i, [vp, i, vp, i])
    assert _abi.PROTOTYPES["vc_debug_sqp_breakdown"] == (i, [vp, i, i, i])


def test_library_exports_regularization_entry_points():
    from vcmpc import _abi
    lib = _abi.load_library()
    for name in ("vc_set_sqp_regularization", "vc_get_sqp_regularization", "vc_debug_sqp_breakdown"):
        assert hasattr(lib, name)
    assert lib.vc_abi_version() == 13
    assert lib.vc_params_sizeof() == ctypes.sizeof(_abi.vc_params) == 1032  # vc_params as it was
    # a null context is an argument error, not a crash
    assert lib.vc_set_sqp_regularization(None, 3, 10.0) == _abi.VC_E_ARG
    assert lib.vc_get_sqp_regularization(None, 0, None, _abi.VC_HOST_PTRS) == _abi.VC_E_ARG
    assert lib.vc_debug_sqp_breakdown(None, 0, 0, 1) == _abi.VC_E_ARG
