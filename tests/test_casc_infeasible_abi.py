"""CPU: the cascaded SQP infeasibility-detection additions of the C ABI (ABI 13, additive:
vc_set_casc_infeasibility / vc_get_casc_farkas) are declared by include/vcmpc.h, mirrored by
vcmpc._abi and exported by the library; no compute calls."""
import ctypes
import os
import re

from conftest import ROOT


def _header():
    src = open(os.path.join(ROOT, "include", "vcmpc.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_casc_entry_points_and_keeps_abi_13():
    src = _header()
    assert re.search(r"\bint\s+vc_set_casc_infeasibility\s*\(\s*vc_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*double\s+\w+\s*\)", src)
    assert re.search(r"\bint\s+vc_get_casc_farkas\s*\(\s*vc_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*void\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", src)
    assert re.search(r"#define\s+VCMPC_ABI_VERSION\s+13\b", src)
    enum = re.search(r"enum\s+vc_status\s*\{(.*?)\}", src, flags=re.S).group(1)
    assert len(re.findall(r"VC_[A-Z_]+\s*=\s*\d+", enum)) == 5  # no new status value


def test_header_documents_the_cascaded_path():
    src = open(os.path.join(ROOT, "include", "vcmpc.h")).read()
    status_doc = src[src.index("/* VC_INFEASIBLE (ABI 13"):src.index("enum vc_status")]
    assert "vc_set_casc_infeasibility" in status_doc and "vc_get_casc_farkas" in status_doc
    diag_doc = src[src.index("vc_solve plus per-problem solver diagnostics"):src.index("int vc_solve_diag(")]
    assert "vc_set_casc_infeasibility" in diag_doc
    # the row order and the radius R of the criterion are part of the contract
    doc = src[src.index("Infeasibility detection of the cascaded SQP"):src.index("int vc_get_casc_farkas(")]
    assert "12N - 3 + 6" in doc and "2 trust_Fx / S" in doc
    assert "[V >= V_min, Fx <= Peng / V, Fx up, Fx dn, Fy up, Fy dn]" in doc


def test_abi_mirror_has_casc_prototypes():
    from vcmpc import _abi
    assert _abi.ABI_VERSION == 13
    vp = ctypes.c_void_p
    assert _abi.PROTOTYPES["vc_set_casc_infeasibility"] == (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_double])
    assert _abi.PROTOTYPES["vc_get_casc_farkas"] == (ctypes.c_int, [vp, ctypes.c_int, vp, vp, ctypes.c_int])


def test_library_exports_casc_entry_points():
    from vcmpc import _abi
    lib = _abi.load_library()
    assert hasattr(lib, "vc_set_casc_infeasibility") and hasattr(lib, "vc_get_casc_farkas")
    assert lib.vc_abi_version() == 13
    # a null context is an argument error, not a crash
    assert lib.vc_set_casc_infeasibility(None, 1, 0.0) == _abi.VC_E_ARG
    assert lib.vc_get_casc_farkas(None, 0, None, None, _abi.VC_HOST_PTRS) == _abi.VC_E_ARG
