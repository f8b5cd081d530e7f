// wide-input kernels (mlp_wide16.h): the streamed one-launch forward and its dual form, activation = ReLU
#define MLP_WIDE_RELU true
#include "mlp_wide_fwd_launch.h"
