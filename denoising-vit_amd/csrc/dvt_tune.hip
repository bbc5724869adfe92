// dvt_tune_set (include/dvt_hip.h): process-global A/B and tuning switches.  This unit owns no knob: it hands the pair to the
// units that do (dvt_tune.h), in a fixed order.
#include "dvt_common.h"
#include "dvt_tune.h"

extern "C" int dvt_tune_set(int key, int value) {
  if (key == 1) return dvt_vit_tune(value);
  if (key == 2) return dvt_grid_tune(value);
  if (key == 3) return dvt_adam_tune(value);
  if (key == 18) return dvt_s2_tune(value);
  // key 4 is shared by value: the 128 x 128 unit claims 10 / 11 before the ring takes every value that is left
  for (int (*unit)(int, int) : {gemm_f32_tune, gemm_f32_big_tune, gemm_f32_glds_tune, fit_tune, fit_fused_tune}) {
    const int rc = unit(key, value);
    if (rc != DVT_TUNE_NOT_MINE) return rc;
  }
  return DVT_E_BADARG;
}
