// Explicit instantiation of the MFMA convolution launchers for ElemF16X3 (f16
// operands split into hi + lo, three MFMAs per k16 step - pm_common.h).
#define PM_INSTANTIATE
#include "pm_launch.h"
template hipError_t pm_launch_pair<ElemF16X3>(int, int, bool, const PairArgs&, hipStream_t);
template hipError_t pm_launch_single<ElemF16X3>(int, int, int, const SingleArgs&, hipStream_t);
template hipError_t pm_launch_block3<ElemF16X3>(const PmLaunch&, const PmStage&, int, hipStream_t);
template hipError_t pm_launch_mrf<ElemF16X3>(const PmLaunch&, const PmStage&, hipStream_t);
