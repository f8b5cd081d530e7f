// mlp_update2_dual_kernel<RELU=true, LN=0, WIDE_A 0..1, WIDE_C 0..1> — actor + critic update in one launch (mlp_upd2.h)
#define MLP_UPD_RELU true
#define MLP_UPD_LN 0
#include "mlp_upd2d_launch.h"
