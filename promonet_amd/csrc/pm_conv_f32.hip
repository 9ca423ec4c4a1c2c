// Explicit instantiation of the MFMA convolution launchers for ElemF32.
#define PM_INSTANTIATE
#define PM_INSTANTIATE_STFT
#include "pm_launch.h"
template hipError_t pm_launch_pair<ElemF32>(int, int, bool, const PairArgs&, hipStream_t);
template hipError_t pm_launch_single<ElemF32>(int, int, int, const SingleArgs&, hipStream_t);
template hipError_t pm_launch_block3<ElemF32>(const PmLaunch&, const PmStage&, int, hipStream_t);
template hipError_t pm_launch_mrf<ElemF32>(const PmLaunch&, const PmStage&, hipStream_t);
