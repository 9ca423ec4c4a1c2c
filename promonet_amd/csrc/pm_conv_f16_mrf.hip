// The whole-MRF launchers for ElemF16 in a translation unit of their own: these
// kernels alternate short MFMA loops with VALU-bound epilogues, and the
// max-ilp scheduling strategy (Makefile: MRF_FLAGS) is worth 2.4 % on them
// (profiles/r03/ab_skew.txt) while it costs the other conv kernels up to 1 %.
// They also keep the grouped MFMA loop (PM_MMA_ORDER 0, pm_conv.h): with
// groups of two steps and this scheduler the per-step A loads measured 4.8 %
// slower on `mrf_c32` (profiles/mma_issue/ab_visit1.txt).
#define PM_MMA_ORDER 0
#define PM_INSTANTIATE
#include "pm_launch.h"
template hipError_t pm_launch_mrf<ElemF16>(const PmLaunch&, const PmStage&, hipStream_t);
