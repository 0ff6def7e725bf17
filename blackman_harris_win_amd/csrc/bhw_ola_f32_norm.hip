// bhw_ola_f32_norm.hip -- weighted overlap-add with float32 samples divided by the window envelope (BHW_OLA_NORMALIZE; the kernels
// and their rules: bhw_ola_f32.h).  A unit of its own so that it compiles in parallel with the plain half (bhw_ola_f32.hip).
#include "bhw_ola_f32.h"

int bhwk_ola_f32_norm(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwOlaPlan &pl, const bhw_ola *o,
                      const float *d_y, float *d_x, const int32_t *d_table, const BhwLenPhase *lp, const BhwOlaBatch &bt)
{
    return ola_f32_launch<true>(l, c, w, pl, o, d_y, d_x, d_table, lp, bt);
}
