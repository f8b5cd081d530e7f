// rollout_spread_rec.hip — the one-launch rollout episode of a recurrent shared policy on the GPU-resident simple_spread
// environment (see rollout_spread_rec.h): gru_step3_tiles of gru_step3.h with the trunks' weights in LDS (mlp_ep16l.h)
#include "mlp_host.h"
#include "rollout_spread_rec.h"
