// mlp_update2_dual_kernel<RELU=false, LN=1, WIDE_A 0..1, WIDE_C 0..1> — actor + critic update in one launch (mlp_upd2.h)
#define MLP_UPD_RELU false
#define MLP_UPD_LN 1
#include "mlp_upd2d_launch.h"
