// Explicit instantiation of the MFMA convolution launchers for ElemF16.
#define PM_INSTANTIATE
#include "pm_launch.h"
template hipError_t pm_launch_pair<ElemF16>(int, int, bool, const PairArgs&, hipStream_t);
template hipError_t pm_launch_single<ElemF16>(int, int, int, const SingleArgs&, hipStream_t);
template hipError_t pm_launch_block3<ElemF16>(const PmLaunch&, const PmStage&, int, hipStream_t);
