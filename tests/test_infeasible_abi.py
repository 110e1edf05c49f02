"""CPU: the infeasibility-detection additions of the C ABI (ABI 13, additive) are declared by
include/vcmpc.h, mirrored by vcmpc._abi and exported by the library; no compute calls."""
import ctypes
import os
import re

from conftest import ROOT


def _header():
    src = open(os.path.join(ROOT, "include", "vcmpc.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_infeasible_status_and_entry_points():
    src = _header()
    enum = re.search(r"enum\s+vc_status\s*\{(.*?)\}", src, flags=re.S).group(1)
    vals = {k: int(v) for k, v in re.findall(r"(VC_[A-Z_]+)\s*=\s*(\d+)", enum)}
    assert vals == {"VC_SOLVED": 0, "VC_MAX_ITER": 1, "VC_NONFINITE": 2, "VC_OUT_OF_DOMAIN": 3, "VC_INFEASIBLE": 4}
    assert re.search(r"\bint\s+vc_set_infeasibility\s*\(\s*vc_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*double\s+\w+\s*\)", src)
    assert re.search(r"\bint\s+vc_get_farkas\s*\(\s*vc_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*void\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", src)
    assert re.search(r"#define\s+VCMPC_ABI_VERSION\s+13\b", src)


def test_abi_mirror_has_status_and_prototypes():
    from vcmpc import _abi
    assert _abi.VC_INFEASIBLE == 4
    assert _abi.STATUS_NAMES[4] == "infeasible"
    assert _abi.ABI_VERSION == 13
    vp = ctypes.c_void_p
    assert _abi.PROTOTYPES["vc_set_infeasibility"] == (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_double])
    assert _abi.PROTOTYPES["vc_get_farkas"] == (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_int])


def test_library_exports_infeasibility_entry_points():
    from vcmpc import _abi
    lib = _abi.load_library()
    assert hasattr(lib, "vc_set_infeasibility") and hasattr(lib, "vc_get_farkas")
    assert lib.vc_abi_version() == 13
    # a null context is an argument error, not a crash
    assert lib.vc_set_infeasibility(None, 1, 0.0) == _abi.VC_E_ARG
    assert lib.vc_get_farkas(None, 0, None, _abi.VC_HOST_PTRS) == _abi.VC_E_ARG
