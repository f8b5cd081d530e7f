// mlp_update16_group_kernel<RELU=false, LN=1> — the agents' dual update launches of a separated run in one launch (mlp_upd16.h)
#define MLP_UPD_GROUP
#define MLP_UPD_RELU false
#define MLP_UPD_LN 1
#include "mlp_upd16_launch.h"
