// mlp_update16_md_kernel / mlp_update16_md_dual_kernel<RELU=false, LN=1> — the MultiDiscrete actor on 16-sample tiles (mlp_upd16.h)
#define MLP_UPD_RELU false
#define MLP_UPD_LN 1
#define MLP_UPD_MD
#include "mlp_upd16_launch.h"
