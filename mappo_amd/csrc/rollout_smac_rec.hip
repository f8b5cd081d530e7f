// rollout_smac_rec.hip — the one-launch rollout episode of a recurrent shared policy on SMAC-shaped env output (see
// rollout_smac_rec.h): gru_step3_tiles of gru_step3.h with the trunks' weights in LDS (mlp_ep16l.h) + the SMAC insert per step
#include "mlp_host.h"
#include "rollout_smac_rec.h"
