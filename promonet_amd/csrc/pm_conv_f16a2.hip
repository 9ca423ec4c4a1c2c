// Explicit instantiation of the MFMA convolution launchers for ElemF16A2 (f16
// operands, the ACTIVATIONS split into hi + lo: two MFMAs per k16 step sharing
// one weight fragment - pm_common.h).
#define PM_INSTANTIATE
#include "pm_launch.h"
template hipError_t pm_launch_pair<ElemF16A2>(int, int, bool, const PairArgs&, hipStream_t);
template hipError_t pm_launch_single<ElemF16A2>(int, int, int, const SingleArgs&, hipStream_t);
template hipError_t pm_launch_block3<ElemF16A2>(const PmLaunch&, const PmStage&, int, hipStream_t);
template hipError_t pm_launch_mrf<ElemF16A2>(const PmLaunch&, const PmStage&, hipStream_t);
