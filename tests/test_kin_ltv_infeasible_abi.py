"""CPU: the condensed kinematic kernel is built with and without the in-kernel infeasibility
detection (csrc/kin_ltv.hip, csrc/kin_ltv_det.hip): the library registers kin_ltv_kernel<20, true>
next to kin_ltv_kernel<20, false>.  The feature adds no entry point and keeps ABI 13; the header says
where the detection runs (vc_qp.solver = 2).  No compute calls."""
import os
import re

from conftest import ROOT


def _library_bytes():
    from vcmpc import _abi
    _abi.load_library()  # the library the package uses exists and loads
    with open(_abi.LIB_PATH, "rb") as f:
        return f.read()


def test_library_registers_both_instantiations():
    blob = _library_bytes()
    names = set(m.decode() for m in re.findall(rb"_ZN2vc\w*kin_ltv_kernelILi20ELb[01]EE\w*", blob))
    assert any("kin_ltv_kernelILi20ELb1EE" in n for n in names), sorted(names)
    assert any("kin_ltv_kernelILi20ELb0EE" in n for n in names), sorted(names)


def test_header_documents_the_condensed_detection_and_keeps_abi_13():
    src = open(os.path.join(ROOT, "include", "vcmpc.h")).read()
    assert re.search(r"#define\s+VCMPC_ABI_VERSION\s+13\b", src)
    solver_doc = src[src.index("int32_t solver;"):src.index("int32_t kin_sqp;")]
    assert "2 = as 0, but vc_set_infeasibility" in solver_doc
    set_doc = src[src.index("/* Infeasibility detection (ABI 13, additive)."):src.index("int vc_set_infeasibility(")]
    assert "vc_qp.solver = 2" in set_doc
    status_doc = src[src.index("/* VC_INFEASIBLE (ABI 13"):src.index("enum vc_status")]
    assert "vc_qp.solver = 2" in status_doc
    diag_doc = src[src.index("vc_solve plus per-problem solver diagnostics"):src.index("int vc_solve_diag(")]
    assert "vc_set_infeasibility" in diag_doc and "bit 32" in diag_doc
