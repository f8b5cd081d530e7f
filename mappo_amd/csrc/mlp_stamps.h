// mlp_stamps.h — per-phase cycle stamps of the update kernels (mlp_upd.h, mlp_upd2.h, mlp_upd16.h).
#pragma once
// ------------------------------------------------------------------------------------------------
// diagnostic build only (-DMLP_STAMPS, scripts/stamps.py): per-phase cycle shares of the update kernel.
// In the product build STAMP() expands to nothing and no stamp executes.
// ------------------------------------------------------------------------------------------------
#ifdef MLP_STAMPS
#define N_STAMPS 24
#define STAMP_DECL unsigned long long st_acc_[N_STAMPS] = {}; unsigned long long st_prev_ = __builtin_readcyclecounter();
#define STAMP(i)                                                          \
  do {                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                    \
    const unsigned long long now_ = __builtin_readcyclecounter();         \
    st_acc_[i] += now_ - st_prev_;                                        \
    st_prev_ = now_;                                                      \
    __builtin_amdgcn_sched_barrier(0);                                    \
  } while (0)
#define STAMP_FLUSH()                                                                     \
  do {                                                                                    \
    if (p.stamps && threadIdx.x == 0)                                                     \
      for (int i_ = 0; i_ < N_STAMPS; ++i_) p.stamps[blockIdx.x * N_STAMPS + i_] = st_acc_[i_]; \
  } while (0)
// opt-in (mappo_debug_set_stamps_waves, a buffer of its own): every wave its own row [gridDim.x][blockDim.x / WAVE][N_STAMPS]
// (update16_body: the slowest wave is the one to read), the last slot holding `tag`
#define STAMP_FLUSH_WAVES(tag)                                                                                     \
  do {                                                                                                             \
    if (p.stamps_waves && (threadIdx.x & (WAVE - 1)) == 0) {                                                       \
      unsigned long long *row_ = p.stamps_waves + ((size_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE) * N_STAMPS; \
      for (int i_ = 0; i_ < N_STAMPS - 1; ++i_) row_[i_] = st_acc_[i_];                                         \
      row_[N_STAMPS - 1] = (tag);                                                                                  \
    }                                                                                                              \
  } while (0)
#else
#define STAMP_DECL
#define STAMP(i) do { } while (0)
#define STAMP_FLUSH() do { } while (0)
#define STAMP_FLUSH_WAVES(tag) do { } while (0)
#endif
