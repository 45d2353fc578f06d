// k_solve family 4: simulations that store their commit log (see ks_solve.hip: launch_family, SLOG)
#define KS_TU 4
#include "ks_solve.hip"
