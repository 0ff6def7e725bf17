// bhw_ola_f32.hip -- weighted overlap-add with float32 samples, the plain sum (the kernels and their rules: bhw_ola_f32.h); the
// envelope-normalised half is compiled by bhw_ola_f32_norm.hip.
#include "bhw_ola_f32.h"

int bhwk_ola_f32(const BhwLaunch &l, const BhwCordicCfg &c, const BhwWinCfg &w, const BhwOlaPlan &pl, const bhw_ola *o, bool normalize,
                 const float *d_y, float *d_x, const int32_t *d_table, const BhwLenPhase *lp, const BhwOlaBatch &bt)
{
    if (normalize) return bhwk_ola_f32_norm(l, c, w, pl, o, d_y, d_x, d_table, lp, bt);
    return ola_f32_launch<false>(l, c, w, pl, o, d_y, d_x, d_table, lp, bt);
}
