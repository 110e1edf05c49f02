// st_sqp_reg.hip -- the REG instantiations of st_sqp_kernel (st_sqp.hip): the regularised retry of a
// QP whose interior point breaks down (vc_set_sqp_regularization) and the breakdown
// test hook (vc_debug_sqp_breakdown).  A translation unit of its own so that the two sets of
// instantiations compile side by side and the kernels of a context without the feature are the
// REG = false ones, untouched by it.
#define VC_ST_SQP_REG 1
#include "st_sqp.hip"
