// kin_ltv_det.hip -- the DET instantiation of kin_ltv_kernel (kin_ltv.hip): the condensed kinematic
// kernel with the in-kernel infeasibility detection (vc_set_infeasibility on a vc_qp.solver = 2
// context).  A translation unit of its own so that the two instantiations compile side
// by side and the kernel of a context without the detection is the DET = false one, compiled exactly
// as it is without this file.
#define VC_KIN_LTV_DET 1
#include "kin_ltv.hip"
