// inputs beyond 512 columns (mlp_wide_sliced.h): the one-launch forward, activation = ReLU
#define MLP_WIDE_RELU true
#include "mlp_wide_sliced_launch.h"
