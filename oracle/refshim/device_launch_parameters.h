/* oracle/refshim/device_launch_parameters.h -- threadIdx / blockIdx / blockDim / gridDim live in
 * the shim's cuda_runtime.h (TEST INFRASTRUCTURE ONLY). */
#ifndef MFSR_REFSHIM_DEVICE_LAUNCH_PARAMETERS_H
#define MFSR_REFSHIM_DEVICE_LAUNCH_PARAMETERS_H
#include "cuda_runtime.h"
#endif
