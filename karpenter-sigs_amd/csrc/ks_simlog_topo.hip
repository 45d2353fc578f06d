// k_solve family 5: simulations + topology that store their commit log (see ks_solve.hip: launch_family, SLOG)
#define KS_TU 5
// as ks_sim_topo.hip
#define KS_NODE_K 1
#include "ks_solve.hip"
