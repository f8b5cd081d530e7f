// inputs beyond 512 columns (mlp_wide_sliced.h): the one-launch forward, activation = tanh
#define MLP_WIDE_RELU false
#include "mlp_wide_sliced_launch.h"
